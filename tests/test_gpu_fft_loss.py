"""-m gpu: the frequency-domain loss term (k_fft_loss.hip; m2t_rfft2, m2t_fft_loss_tensor, m2t_fft_loss, losses.fft_loss,
TrainStep(lambda_fft=...)) against the fp64 restatement tests/fft_loss_ref.py.

Inputs stay off the L1 kink: every non-self-conjugate component of the fp64 spectrum is asserted to be at least 1e-5 of the RMS of
those components (a condition on the inputs, checked on what is actually run; a violation fails the test).  One flipped sign of a
component near 0 changes every pixel of the gradient, in any fp32 transform, torch's included.

The gate is not a constant: it is 8 x the error of torch's OWN fp32 rfft2 pipeline against the same fp64 reference on the listed
cases (a different factorisation order and another order of the sign sums change the constant, not the order of magnitude), capped
at the project's fp32 gate 2e-5; value relative, spectrum and gradient as max-abs over the reference's max-abs.  Where the
destination held something before, the single fp32 add contributes half an ulp of the sum on top (HALF_ULP x max |prefill + ref|).

Measured (floor = torch's fp32 error on the CPU, gate = 8 x floor): see the printed lines and DESIGN.md."""
import ctypes as C
import functools

import pytest
import torch

from tests import fft_loss_ref as R
from tests.gpu_util import assert_flat_equal
from tests.test_gpu_pixel_loss import _backward, _forward, _images, _model, _srpre

pytestmark = pytest.mark.gpu

ARG, STATE = -2, -3
LAM = 0.1
HALF_ULP = 6e-8          # 2^-24 = 5.96e-8
MARGIN = 1e-5
FP32_GATE = 2e-5
# (H, W), seed of the recipe, seed of the 10 % pushed outside [0, 1] for the clamp run (found on the CPU so that the precondition
# holds after the push).  radix 2 only | radix 3 in H | radix 3 in W | H < W with radix 3 in H | H > W | three LDS strips of 16 kx
CASES = [((16, 16), 0, 100), ((24, 32), 1, 100), ((32, 48), 0, 101), ((36, 64), 4, 100), ((48, 24), 0, 100), ((96, 64), 0, 100)]
IDS = [f"{h}x{w}" for (h, w), _, _ in CASES]


def _lib_():
    from m2trans_amd import _lib
    return _lib, _lib.load()


@functools.lru_cache(maxsize=None)
def _gates():
    """(spectrum, value, gradient) gates: 8 x the largest error of torch's fp32 pipeline over the listed cases, capped at 2e-5."""
    floors = [R.torch_fp32_floor(*R.inputs(*shape, seed)) for shape, seed, _ in CASES]
    floor = [max(f[i] for f in floors) for i in range(3)]
    gates = tuple(min(8.0 * f, FP32_GATE) for f in floor)
    print("torch fp32 floor (spectrum, value, gradient): " + ", ".join(f"{f:.3e}" for f in floor)
          + "; gates: " + ", ".join(f"{g:.3e}" for g in gates))
    assert all(0.0 < f < 1e-6 for f in floor), floor
    return gates


def _scratch(lib, B, Cn, H, W, poison=False):
    n = lib.m2t_fft_loss_scratch_bytes(B, Cn, H, W)
    assert n > 0
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    if poison:
        t.fill_(0xFF)
    return t


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------ 1. the plain transform
@pytest.mark.parametrize("norm", ["backward", "ortho"])
@pytest.mark.parametrize("shape,seed,_push", CASES, ids=IDS)
def test_rfft2_against_torch_fft_in_fp64(shape, seed, _push, norm):
    _lib, lib = _lib_()
    H, W = shape
    x, y = R.inputs(H, W, seed)
    d = (x - y).contiguous()                                          # fp32, the difference the loss transforms
    want = torch.view_as_real(torch.fft.rfft2(d.double(), norm=norm))
    planes = d.shape[0] * d.shape[1]
    out = torch.full((planes, H, W // 2 + 1, 2), float("nan"), device="cuda")
    dd = d.cuda()
    _lib.check(lib.m2t_rfft2(_lib.ptr(dd), _lib.ptr(out), planes, H, W, R.NORMS[norm], _lib.stream_ptr()), "m2t_rfft2")
    torch.cuda.synchronize()
    got = out.cpu().view(*d.shape[:2], H, W // 2 + 1, 2)
    assert bool(torch.isfinite(got).all())
    err = _rel(got.double(), want)
    print(f"rfft2 {H}x{W} {norm}: error {err:.3e} (gate {_gates()[0]:.3e})")
    assert err <= _gates()[0], err
    sc = R.self_conjugate_mask(H, W)
    im = got[..., 1][..., sc]
    assert im.numel() == planes * 4 and bool((im.view(torch.int32) == 0).all()), "self-conjugate imaginary parts must be +0.0"


# ------------------------------------------------------------------ 2. the plan-free entry
def _run_tensor(lib, _lib, xbuf, yd, shape, layout, clamp, norm, scale, prefill, loss_prefill, accumulate, scratch, with_grad=True):
    B, Cn, H, W = shape
    rows, rs = layout
    gbuf = torch.full((B, Cn, rows, rs), float("nan"))                # what lies outside [H, W] is never written
    gbuf[..., :H, :W] = prefill
    gbuf = gbuf.cuda()
    loss = torch.full((1,), loss_prefill, device="cuda")
    rc = lib.m2t_fft_loss_tensor(_lib.ptr(xbuf), _lib.ptr(yd), B, Cn, H, W, Cn * rows * rs, rs, 1.0, clamp, R.NORMS[norm], scale,
                                 _lib.ptr(gbuf) if with_grad else None, _lib.ptr(loss), accumulate, _lib.ptr(scratch), _lib.stream_ptr())
    _lib.check(rc, "m2t_fft_loss_tensor")
    torch.cuda.synchronize()
    return gbuf.cpu(), loss.cpu()


def _check_tensor(x, y, clamp, norm, layout=None):
    _lib, lib = _lib_()
    B, Cn, H, W = x.shape
    shape = tuple(x.shape)
    rows, rs = layout or (H, W)
    tag = f"{shape} clamp {clamp} {norm} layout {rows}x{rs}"
    margin = R.kink_margin((x.double().clamp(0, 1) if clamp else x.double()) - y.double())
    assert margin >= MARGIN, f"{tag}: the inputs sit on the L1 kink ({margin:.2e} of the RMS)"
    scale = 0.37 / (2 * B * Cn * H * (W // 2 + 1))
    want_loss, want = R.value_and_grad(x, y, 1.0, bool(clamp), scale, norm)
    gmax = float(want.abs().max())
    assert gmax > 0
    _, g_val, g_grad = _gates()
    nan = float("nan")
    xbuf = torch.full((B, Cn, rows, rs), nan)                         # what lies outside [H, W] must never be read ...
    xbuf[..., :H, :W] = x
    xbuf, yd = xbuf.cuda(), y.cuda()
    inside = torch.zeros((B, Cn, rows, rs), dtype=torch.bool)
    inside[..., :H, :W] = True
    run = functools.partial(_run_tensor, lib, _lib, xbuf, yd, shape, (rows, rs), clamp, norm, scale)
    g0, l0 = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W))
    got = g0[..., :H, :W].double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(l0).all()), tag
    err, verr = _rel(got, want), abs(float(l0) - float(want_loss)) / abs(float(want_loss))
    print(f"{tag}: margin {margin:.2e}; gradient error {err:.3e} (gate {g_grad:.3e}); value {float(l0):.9e} against {float(want_loss):.9e}: "
          f"{verr:.3e} (gate {g_val:.3e})")
    assert err <= g_grad, (tag, err)
    assert verr <= g_val, (tag, verr)
    if clamp:
        outside = (x < 0) | (x > 1)
        assert 0.05 < float(outside.double().mean()) < 0.15, tag
        assert bool((g0[..., :H, :W][outside].view(torch.int32) == 0).all()), f"{tag}: something was added where the clamp is active"
    # outside [H, W]: bit-unchanged
    assert torch.equal(g0.view(torch.int32)[~inside], torch.full((B, Cn, rows, rs), nan).view(torch.int32)[~inside]), tag
    # two runs, and a run on NaN-poisoned scratch: bit-identical
    for poison in (False, True):
        g1, l1 = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W, poison))
        assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)) and torch.equal(l1, l0), (tag, poison)
    # value only (gx_add = NULL): the same value
    _, lv = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W), with_grad=False)
    assert torch.equal(lv, l0), tag
    # a non-zero destination is added to, in the gradient and (accumulate = 1) in the value
    g = torch.Generator().manual_seed(7)
    noise = (torch.randn((B, Cn, H, W), generator=g) * gmax).float()
    g2, l2 = run(noise, 2.5, 1, _scratch(lib, B, Cn, H, W))
    sum_ref = noise.double() + want
    excess = float((g2[..., :H, :W].double() - sum_ref).abs().max()) - (g_grad * gmax + HALF_ULP * float(sum_ref.abs().max()))
    assert excess <= 0.0, (tag, excess)
    mask = ~((x < 0) | (x > 1)) if clamp else torch.ones_like(x, dtype=torch.bool)
    assert torch.equal(g2[..., :H, :W][mask], (noise + g0[..., :H, :W])[mask]), tag          # (the same fp32 add)
    assert torch.equal(g2[..., :H, :W][~mask].view(torch.int32), noise[~mask].view(torch.int32)), tag
    assert torch.equal(l2, torch.tensor([2.5]) + l0), (tag, float(l2), float(l0))


@pytest.mark.parametrize("shape,seed,_push", CASES, ids=IDS)
def test_plan_free_entry_against_fp64(shape, seed, _push):
    x, y = R.inputs(*shape, seed)
    _check_tensor(x, y, 0, "backward")


@pytest.mark.parametrize("shape,seed,push", [c for c in CASES if c[2] is not None], ids=[i for i, c in zip(IDS, CASES) if c[2] is not None])
def test_plan_free_entry_through_the_clamp_on_a_strided_image(shape, seed, push):
    """clamp = 1 with about 10 % of x pushed outside [0, 1] (those pixels get exactly no addition), x and the destination in a padded
    buffer (row stride W + 16, H + 8 rows per channel) whose elements outside [H, W] are NaN and stay untouched; norm "ortho"."""
    H, W = shape
    x, y = R.inputs(H, W, seed, push_seed=push)
    _check_tensor(x, y, 1, "ortho", layout=(H + 8, W + 16))


def test_plan_free_entry_on_one_plane():
    x, y = R.inputs(24, 32, 0, B=1, C=1)
    _check_tensor(x, y, 0, "backward")


# ------------------------------------------------------------------ 3. the autograd Function
def test_fft_loss_function_gradient_and_errors():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import FFTLoss, fft_loss
    x, y = R.inputs(36, 64, 4)
    assert R.kink_margin(x.double() - y.double()) >= MARGIN
    _, g_val, g_grad = _gates()
    for norm in ("backward", "ortho"):
        want, want_g = R.value_and_grad(x, y, 1.0, False, None, norm)
        leaf = x.cuda().requires_grad_(True)
        got = fft_loss(leaf, y.cuda(), norm=norm)
        (got * 3.0).backward()                                        # (an upstream factor reaches the gradient)
        torch.cuda.synchronize()
        assert got.shape == () and abs(float(got) - float(want)) <= g_val * abs(float(want))
        err = _rel(leaf.grad.double().cpu() / 3.0, want_g)
        print(f"fft_loss Function {norm}: gradient error {err:.3e} (gate {g_grad:.3e})")
        assert err <= g_grad, err
        assert float(FFTLoss(norm=norm)(x.cuda(), y.cuda())) == float(got)
    with pytest.raises(M2TError, match="HIP device"):
        fft_loss(x, y)                                                # host tensors: no fallback
    with pytest.raises(M2TError):
        fft_loss(x.cuda(), y.cuda().requires_grad_(True))
    for H, W in ((40, 56), (160, 224)):
        z = torch.zeros(1, 3, H, W, device="cuda")
        with pytest.raises(M2TError, match=rf"{H}x{W}.*2\^a \* 3\^b"):
            fft_loss(z, z)
    with pytest.raises(M2TError):
        fft_loss(x.cuda(), y.cuda(), norm="forward")


# ------------------------------------------------------------------ 4. the plan entry
def _reals(hr):
    return 2 * hr.shape[0] * 3 * hr.shape[-2] * (hr.shape[-1] // 2 + 1)


def _pixel(lib, plan, hr, out, weight=1.0, divisor=None, deferred=False):
    from m2trans_amd import _lib
    fn = lib.m2t_pixel_loss_deferred if deferred else lib.m2t_pixel_loss
    return fn(plan.handle, 0, 0.0, _lib.ptr(hr), weight, float(hr.numel() if divisor is None else divisor), 1.0, _lib.ptr(out),
              _lib.ptr(plan.workspace), _lib.stream_ptr())


def _fft(lib, plan, hr, out, weight=LAM, divisor=None, accumulate=0, scratch=None, norm="backward"):
    from m2trans_amd import _lib
    if scratch is None:
        scratch = _scratch(lib, hr.shape[0], 3, hr.shape[-2], hr.shape[-1])
    rc = lib.m2t_fft_loss(plan.handle, _lib.ptr(hr), weight, float(_reals(hr) if divisor is None else divisor), 1.0, R.NORMS[norm],
                          _lib.ptr(out), accumulate, _lib.ptr(scratch), _lib.ptr(plan.workspace), _lib.stream_ptr())
    torch.cuda.synchronize()             # (the scratch of this helper dies with the call)
    return rc


def _ssim(lib, plan, hr, out, weight=LAM):
    from m2trans_amd import _lib
    B, _, Hs, Ws = hr.shape
    scratch = torch.empty(lib.m2t_ssim_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    rc = lib.m2t_ssim_loss(plan.handle, _lib.ptr(hr), weight, float(B * 3 * (Hs - 10) * (Ws - 10)), 1.0, _lib.ptr(out), 0, _lib.ptr(scratch),
                           _lib.ptr(plan.workspace), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


LR = (18, 24)            # the smallest LR images a plan takes are 17 x 17; 18 x 24 gives SR sizes 2^a 3^b at every scale, reflect-padded to 32 x 32


# (dtype, scale, seed of the perturbation e: its own spectrum keeps 5e-5 of the RMS at the SR shape, found on the CPU)
@pytest.mark.parametrize("dtype,scale,eseed", [("bf16", 4, 3), ("fp32", 2, 3), ("bf16", 3, 12)], ids=["bf16-x4-72x96", "fp32-x2-36x48", "bf16-x3-54x72"])
def test_plan_entry_adds_the_seed_against_fp64(dtype, scale, eseed):
    """The forward's own pre-clamp output is read back and hr = clamp(sr) - e with e = 0.1 randn, so that d is e up to fp32 rounding
    and stays off the kink (asserted on the actual d).  m2t_pixel_loss(weight 0) materialises a zero seed: after m2t_fft_loss it is
    the reference gradient, exactly 0 in the reflect padding and where the clamp is active; behind the L1 seed (weight 1) it is the
    L1 seed plus the reference."""
    _lib, lib = _lib_()
    B, (H, W) = 2, LR
    model = _model(scale, dtype, 2)
    x, _ = _images(B, H, W, scale)
    plan = model._plan_for(x)
    _forward(lib, model, plan, x)
    torch.cuda.synchronize()
    pre = _srpre(plan, B, scale).clone().cpu()
    Hs, Ws = H * scale, W * scale
    assert pre.shape[-2] > Hs and pre.shape[-1] > Ws, "the plan is meant to be reflect-padded"
    g = torch.Generator().manual_seed(eseed)
    e = 0.1 * torch.randn(B, 3, Hs, Ws, generator=g, dtype=torch.float64)
    inner = pre[..., :Hs, :Ws]
    hr_cpu = (inner.double().clamp(0, 1) - e).float().contiguous()
    margin = R.kink_margin(inner.double().clamp(0, 1) - hr_cpu.double())
    tag = f"{dtype} x{scale} SR {Hs}x{Ws}"
    assert margin >= MARGIN, f"{tag}: the inputs sit on the L1 kink ({margin:.2e} of the RMS)"
    hr = hr_cpu.cuda()
    pad = torch.ones(pre.shape, dtype=torch.bool)
    pad[..., :Hs, :Ws] = False
    clamped = (pre < 0) | (pre > 1)
    _, g_val, g_grad = _gates()
    l1, out = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    for norm in ("backward", "ortho"):
        want_loss, want = R.loss_and_seed(pre, hr_cpu, weight=LAM, divisor=_reals(hr), norm=norm)
        gmax = float(want.abs().max())
        # the term alone, on a zero seed
        gpre.fill_(float("nan"))
        assert _pixel(lib, plan, hr, l1, weight=0.0) == 0 and _fft(lib, plan, hr, out, norm=norm) == 0
        got = gpre.view(pre.shape).cpu()
        assert bool(torch.isfinite(got).all()), tag
        assert int(torch.count_nonzero(got[pad])) == 0, f"{tag}: seed in the padding"
        assert int(torch.count_nonzero(got[clamped])) == 0, f"{tag}: seed where the clamp is active"
        err, verr = _rel(got.double(), want), abs(float(out) - float(want_loss)) / abs(float(want_loss))
        print(f"{tag} {norm}: margin {margin:.2e}, clamped share {float(clamped.double().mean()):.3f}; seed error {err:.3e} (gate {g_grad:.3e}); "
              f"value {float(out):.9e} against {float(want_loss):.9e}: {verr:.3e} (gate {g_val:.3e})")
        assert err <= g_grad and verr <= g_val, (tag, norm, err, verr)
        # behind the L1 seed: seed before + the reference
        gpre.fill_(float("nan"))
        assert _pixel(lib, plan, hr, l1, weight=1.0) == 0
        torch.cuda.synchronize()
        before = gpre.view(pre.shape).cpu().clone()
        assert _fft(lib, plan, hr, out, norm=norm) == 0
        got = gpre.view(pre.shape).cpu()
        sum_ref = before.double() + want
        excess = float((got.double() - sum_ref).abs().max()) - (g_grad * gmax + HALF_ULP * float(sum_ref.abs().max()))
        assert excess <= 0.0, (tag, norm, excess)
        assert int(torch.count_nonzero(got[pad])) == 0 and int(torch.count_nonzero(got[clamped])) == 0, tag


def test_plan_entry_state_and_argument_errors():
    """State rules of m2t_ssim_loss; argument errors; an SR size outside the rule (LR 20 x 28 at x2: 40 x 56) is refused by the entry
    before any launch and by TrainStep with an M2TError that names the size and the rule."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    model = _model(4, "fp32", 1)
    x, hr = _images(1, *LR, 4)
    plan = model._plan_for(x)
    out = torch.zeros(1, device="cuda")
    assert _fft(lib, plan, hr, out) == STATE                         # before a forward
    _forward(lib, model, plan, x)
    assert _fft(lib, plan, hr, out) == STATE                         # before any seed
    assert _pixel(lib, plan, hr, out, deferred=True) == 0
    assert _fft(lib, plan, hr, out) == STATE                         # a deferred request leaves no materialised seed
    assert b"materialised" in lib.m2t_last_error_string()
    assert _pixel(lib, plan, hr, out) == 0
    assert _fft(lib, plan, hr, out) == 0
    scratch = _scratch(lib, 1, 3, hr.shape[-2], hr.shape[-1])
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    for bad in (dict(hr=None), dict(out=None), dict(scratch=None), dict(ws=None), dict(R=0.0), dict(div=0.0), dict(div=float("nan")),
                dict(norm=2), dict(norm=-1)):
        a = dict(hr=_lib.ptr(hr), out=_lib.ptr(out), scratch=_lib.ptr(scratch), ws=ws, R=1.0, div=float(_reals(hr)), norm=0)
        a.update(bad)
        assert lib.m2t_fft_loss(plan.handle, a["hr"], LAM, a["div"], a["R"], a["norm"], a["out"], 0, a["scratch"], a["ws"], st) == ARG, bad
    torch.cuda.synchronize()
    # an unsupported SR size
    m2 = _model(2, "fp32", 1)
    x2, hr2 = _images(1, 20, 28, 2)
    p2 = m2._plan_for(x2)
    _forward(lib, m2, p2, x2)
    assert _pixel(lib, p2, hr2, out) == 0
    assert lib.m2t_fft_loss_scratch_bytes(1, 3, 40, 56) == 0
    assert lib.m2t_fft_loss(p2.handle, _lib.ptr(hr2), LAM, 1.0, 1.0, 0, _lib.ptr(out), 0, _lib.ptr(scratch), _lib.ptr(p2.workspace), st) == ARG
    assert b"2^a * 3^b" in lib.m2t_last_error_string()
    torch.cuda.synchronize()
    ts = TrainStep(m2, world_size=1, lambda_fft=LAM)
    with pytest.raises(M2TError, match=r"40x56.*2\^a \* 3\^b"):
        ts.forward_backward(x2, hr2)


# ------------------------------------------------------------------ 5. TrainStep against the sequence by hand
def _by_hand(model, plan, x, hr, lam=LAM, norm="backward", pix_div=None, fft_div=None, with_ssim=False):
    """(l1 [1], ssim [1] or None, fft [1], gradients): m2t_forward -> m2t_pixel_loss (l1) -> [m2t_ssim_loss] -> m2t_fft_loss ->
    m2t_backward into fresh buffers."""
    _lib, lib = _lib_()
    l1, ss, ff = (torch.full((1,), float("nan"), device="cuda") for _ in range(3))
    grads = torch.full_like(model.flat_params, float("nan"))
    _forward(lib, model, plan, x)
    assert _pixel(lib, plan, hr, l1, divisor=pix_div) == 0
    if with_ssim:
        assert _ssim(lib, plan, hr, ss) == 0
    assert _fft(lib, plan, hr, ff, weight=lam, divisor=fft_div, norm=norm) == 0
    _backward(lib, model, plan, x, grads)
    torch.cuda.synchronize()
    return l1, (ss if with_ssim else None), ff, grads


@pytest.mark.parametrize("dtype,scale,norm,with_ssim", [("bf16", 4, "backward", False), ("fp32", 2, "ortho", False), ("bf16", 4, "backward", True)],
                         ids=["bf16-x4", "fp32-x2-ortho", "bf16-x4-with-ssim"])
def test_train_step_is_the_sequence_by_hand(dtype, scale, norm, with_ssim):
    """Two steps with different batches: losses, gradients, parameters and moments bit-identical to m2t_forward -> m2t_pixel_loss ->
    [m2t_ssim_loss ->] m2t_fft_loss -> m2t_backward -> m2t_adam_step on a twin; ts.loss is the sum of the parts."""
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    B, (H, W) = 2, LR
    m_a, m_b = _model(scale, dtype, 2), _model(scale, dtype, 2)
    ts = TrainStep(m_a, lr=1e-4, world_size=1, lambda_fft=LAM, fft_norm=norm, lambda_ssim=LAM if with_ssim else 0.0)
    exp_avg, exp_avg_sq = torch.zeros_like(m_b.flat_params), torch.zeros_like(m_b.flat_params)
    first_grads = None
    for step in range(2):
        x, hr = _images(B, H, W, scale, step)
        loss = ts.step(x, hr)
        torch.cuda.synchronize()
        plan = m_b._plan_for(x)
        l1, ss, ff, grads = _by_hand(m_b, plan, x, hr, norm=norm, with_ssim=with_ssim)
        if step == 0:
            first_grads = grads.clone()
        n = grads.numel()
        _lib.check(lib.m2t_adam_step(_lib.ptr(m_b.flat_params), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), n, 1e-4, 0.9,
                                     0.999, 1e-8, step + 1, 1.0, _lib.stream_ptr()), "m2t_adam_step")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(grads).all()) and float(ff) > 0 and float(l1) > 0
        assert ts.fft_loss.shape == (1,) and ts.fft_loss.is_cuda and ts.fft_loss.dtype == torch.float32
        assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.fft_loss, ff)
        if with_ssim:
            assert torch.equal(ts.ssim_loss, ss) and torch.equal(loss, l1 + ss + ff), (step, float(loss))
        else:
            assert ts.ssim_loss is None and torch.equal(loss, l1 + ff), (step, float(loss))
        assert ts.loss is loss
        assert_flat_equal(m_a, ts.grads, grads, f"gradients, step {step}")
        assert_flat_equal(m_a, m_a.flat_params.detach(), m_b.flat_params.detach(), f"parameters, step {step}")
        assert_flat_equal(m_a, ts.exp_avg, exp_avg, f"exp_avg, step {step}")
        assert_flat_equal(m_a, ts.exp_avg_sq, exp_avg_sq, f"exp_avg_sq, step {step}")
    # the term is live: the step without it gives other gradients
    x, hr = _images(B, H, W, scale, 0)
    ts0 = TrainStep(_model(scale, dtype, 2), world_size=1, lambda_ssim=LAM if with_ssim else 0.0)
    ts0.forward_backward(x, hr)
    torch.cuda.synchronize()
    assert not torch.equal(ts0.grads, first_grads)


def test_accumulated_fft_equals_the_micro_batch_gradients_summed_in_call_order():
    """accum_steps = 2 at micro-batch (1, 18, 24), bf16 x4: the accumulated buffer is the fp32 sum, in call order, of the two micro-batch
    gradients taken by hand with the cycle's divisors (the rule of tests/test_gpu_accum.py); ts.fft_loss is the sum of the two values."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    x, hr = _images(2, *LR, 4)
    m_a, m_b = _model(4, "bf16", 2), _model(4, "bf16", 2)
    ts = TrainStep(m_a, world_size=1, accum_steps=2, lambda_fft=LAM)
    ts.forward_backward(x[0:1], hr[0:1])
    with pytest.raises(M2TError):
        ts.optimizer_step()                                          # in mid-cycle
    with pytest.raises(M2TError):
        ts.set_lambda_fft(0.0)
    loss = ts.forward_backward(x[1:2], hr[1:2])
    torch.cuda.synchronize()
    parts = []
    for i in range(2):
        cx, chr_ = x[i:i + 1].contiguous(), hr[i:i + 1].contiguous()
        parts.append(_by_hand(m_b, m_b._plan_for(cx), cx, chr_, pix_div=hr.numel(), fft_div=_reals(hr)))
    assert float(parts[1][3].abs().max()) > 0 and float(parts[1][2]) > 0
    assert torch.equal(ts.fft_loss, parts[0][2] + parts[1][2]), (float(ts.fft_loss), float(parts[0][2] + parts[1][2]))
    assert torch.equal(ts.l1_loss, parts[0][0] + parts[1][0])
    assert torch.equal(loss, ts.l1_loss + ts.fft_loss)
    assert_flat_equal(m_a, ts.grads, parts[0][3] + parts[1][3], "accumulated L1 + FFT")
    ts.optimizer_step()
    assert ts.micro_count == 0


def test_semantic_grad_route_with_the_fft_term_is_the_sequence_by_hand():
    """TrainStep(lambda_fft, differentiable SemanticLoss with hashed text features) against the sequence by hand (m2t_forward -> encoder
    value and gradient -> m2t_pixel_loss -> m2t_fft_loss -> m2t_add_output_grad -> m2t_backward): bit-identical."""
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
    ts = TrainStep(m_a, world_size=1, semantic_loss=sl, lambda_clip=0.01, lambda_fft=LAM)
    torch.manual_seed(1)
    loss = ts.forward_backward(x, hr, caps)
    torch.cuda.synchronize()
    # by hand
    plan = m_b._plan_for(x)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    sr = torch.empty_like(hr)
    l1, ff = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    g_b = torch.full_like(m_b.flat_params, float("nan"))
    torch.manual_seed(1)
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(m_b.flat_params), _lib.ptr(x), _lib.ptr(sr), 1.0, 1, ws, st), "m2t_forward")
    _, gsem, origins = sl._value_and_grad(sr, hr, caps)
    gsem = gsem.contiguous()
    arr = None if origins is None else (C.c_int * (2 * len(origins)))(*[int(v) for o in origins for v in o])
    assert _pixel(lib, plan, hr, l1) == 0
    assert _fft(lib, plan, hr, ff) == 0
    _lib.check(lib.m2t_add_output_grad(plan.handle, _lib.ptr(gsem), gsem.shape[2], gsem.shape[3], arr, 0.01, 1.0, ws, st), "m2t_add_output_grad")
    _backward(lib, m_b, plan, x, g_b)
    torch.cuda.synchronize()
    assert float(ff) > 0 and bool(torch.isfinite(g_b).all())
    assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.fft_loss, ff)
    assert torch.equal(loss, ts.l1_loss + ts.fft_loss + ts.clip_loss)
    assert_flat_equal(m_a, ts.grads, g_b, "semantic-gradient route with the FFT term")


# ------------------------------------------------------------------ 6. the default step is untouched
@pytest.mark.parametrize("dtype,scale", [("bf16", 4), ("fp32", 2)])
def test_lambda_fft_zero_is_the_default_step_bit_for_bit(dtype, scale):
    from m2trans_amd.train_step import TrainStep
    B, (H, W) = 2, LR
    res = []
    for kw in ({}, {"lambda_fft": 0.0}):
        model = _model(scale, dtype, 2)
        ts = TrainStep(model, lr=1e-4, world_size=1, **kw)
        assert ts.fft_loss is None and ts._fft_scratch == {}
        out = []
        for step in range(2):
            x, hr = _images(B, H, W, scale, step)
            loss = ts.step(x, hr)
            torch.cuda.synchronize()
            assert ts.fft_loss is None and ts._fft_scratch == {} and loss is ts.l1_loss
            out.append((loss.clone(), ts.grads.clone(), model.flat_params.detach().clone()))
        res.append((model, out))
    (model, a), (_, b) = res
    for step in range(2):
        assert torch.equal(a[step][0], b[step][0])
        assert_flat_equal(model, a[step][1], b[step][1], f"gradients, step {step}")
        assert_flat_equal(model, a[step][2], b[step][2], f"parameters, step {step}")
