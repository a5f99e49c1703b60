"""-m gpu: the MS-SSIM loss term (k_msssim_loss.hip; m2t_msssim_loss_tensor, m2t_msssim_loss, losses.ms_ssim_loss,
metrics.ms_ssim_device, TrainStep(lambda_msssim=...)) against the fp64 restatement tests/msssim_loss_ref.py: the plan-free entry per
element, the pyramid bit for bit, the zero rule, the plan entry on the forward's own pre-clamp output, TrainStep against the sequence
composed by hand and against the autograd route, the default step, accumulation, and the three optional terms together.

The gate of a gradient element is |got - ref| <= 1e-6 |ref| + 1e-7 max_bc |ref| + 6e-8 |prefill + ref|: it is derived, not measured.
Everything between the fp32 inputs and the single fp32 rounding is fp64 and the pyramid is exact; what remains is the order of the
fp64 sums (1e-15 of the largest term) and one rounding (6e-8), plus -- where the destination held something -- half an ulp of the sum.

Inputs: HR = smoothed uniform noise, SR = HR + sigma * randn (every level mean positive: asserted through the reference) wherever a
gradient is compared; SR = 1 - HR only for the zero rule.  In the plan and TrainStep tests SR is what the model gives, so HR is built
from the read-back pre-clamp output: HR = clamp(clamp(pre) + 0.05 randn)."""
import ctypes as C

import pytest
import torch

from tests import msssim_loss_ref as R
from tests import pixel_loss_ref as RP
from oracle import m2trans_oracle as O
from tests.gpu_util import assert_flat_equal, build_model
from tests.test_gpu_pixel_loss import _backward, _forward, _images

pytestmark = pytest.mark.gpu

ARG, STATE = -2, -3
LAM = 0.16
NB = 1
HALF_ULP = 6e-8          # 2^-24 = 5.96e-8
# The closed-form parameters give a pre-clamp output within a few hundredths of 0, centred on 0 (the last tail conv has no bias): it
# is scaled (which scales the pre-clamp output exactly) so that, with one block, about half lies below 0, a twelfth above 1 and the
# rest inside -- the plan test reads it back and requires that coverage.
TAIL_GAIN = {4: ("tail.6.weight", 10.0), 3: ("tail.3.weight", 2.0), 2: ("tail.3.weight", 40.0)}
_PARAMS = {}


def _model(scale, dtype, nb=NB):
    if (scale, nb) not in _PARAMS:
        p = {k: v.clone() for k, v in O.closed_form_params(64, scale, nb).items()}
        name, gain = TAIL_GAIN[scale]
        p[name] = p[name] * gain
        _PARAMS[(scale, nb)] = p
    return build_model(scale, nb, dtype, params=_PARAMS[(scale, nb)])[0]


def _lib_():
    from m2trans_amd import _lib
    return _lib, _lib.load()


def _scratch(lib, B, Cn, H, W, poison=False):
    n = lib.m2t_msssim_loss_scratch_bytes(B, Cn, H, W)
    assert n > 0
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    if poison:
        t.fill_(0xFF)
    return t


def _gate(got, ref, prefill=None):
    """(elements beyond the gate, largest |got - want| / bound) for [B,C,H,W] fp64 tensors."""
    top = ref.abs().amax(dim=(-2, -1), keepdim=True)
    want = ref if prefill is None else prefill + ref
    bound = 1e-6 * ref.abs() + 1e-7 * top + HALF_ULP * want.abs()
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), (err > 0).double() * float("inf"))
    return int((err > bound).sum()), float(ratio.max())


# ------------------------------------------------------------------ 1. the plan-free entry against fp64
# (shape, sigma, (rows, row stride) of the buffer that holds x or None = contiguous)
CASES = [((1, 1, 161, 161), 0.02, None),                # every level odd, a 1 x 1 map at level 4
         ((2, 3, 176, 192), 0.3, (180, 200)),           # strided x: row stride 200, image stride 3 * 180 * 200
         ((1, 3, 177, 200), 0.02, (177, 208)),          # mixed parity; x a view with a longer row
         ((1, 1, 200, 560), 0.3, None)]                 # level 4 is 35 wide: two tiles of the coarse kernel, 18 of the fine one
CASE_IDS = ["odd-chain", "strided", "mixed-parity", "wide"]
_REF = {}


def _case(idx, clamp, Rr):
    """Inputs and the reference of one case, computed once and shared (never modified)."""
    key = (idx, clamp, Rr)
    if key not in _REF:
        shape, sigma, _ = CASES[idx]
        x, y = R.smooth_pair(shape, sigma, seed=10 + idx, R=Rr, spill=True)
        outside = float(((x < 0) | (x > Rr)).double().mean())
        assert 0.05 < outside < 0.2, f"{shape}: share of x outside [0, R] {outside}"
        scale = 0.37 / (shape[0] * shape[1])
        loss, grad, M, levels = R.value_and_grad(x, y, Rr, bool(clamp), scale)
        assert bool((M > 0).all()) and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0, (shape, M)
        _REF[key] = (x, y, scale, loss, grad, M, levels)
    return _REF[key]


@pytest.mark.parametrize("Rr", [1.0, 255.0], ids=["R1", "R255"])
@pytest.mark.parametrize("clamp", [0, 1])
@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_plan_free_entry_against_fp64(idx, clamp, Rr):
    _lib, lib = _lib_()
    shape, _, layout = CASES[idx]
    B, Cn, H, W = shape
    x, y, scale, want_loss, want, want_M, _ = _case(idx, clamp, Rr)
    rows, rs = layout or (H, W)
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
        per = torch.full((B * Cn,), nan, dtype=torch.float64, device="cuda")
        rc = lib.m2t_msssim_loss_tensor(_lib.ptr(xbuf), _lib.ptr(yd), B, Cn, H, W, Cn * rows * rs, rs, Rr, clamp, scale,
                                        _lib.ptr(gbuf) if with_grad else None, _lib.ptr(loss), _lib.ptr(per), accumulate,
                                        _lib.ptr(scratch), _lib.stream_ptr())
        _lib.check(rc, "m2t_msssim_loss_tensor")
        torch.cuda.synchronize()
        return gbuf.cpu(), loss.cpu(), per.cpu()

    tag = f"{shape} clamp {clamp} R {Rr:g}"
    g0, l0, p0 = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W))
    got = g0[..., :H, :W].double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(l0).all()), tag
    nbad, worst = _gate(got, want)
    print(f"{tag}: gradient, largest |got - ref| / bound {worst:.3f} (max |ref| {float(want.abs().max()):.3e}); "
          f"value {float(l0):.9e} against {float(want_loss):.9e}; min M {float(want_M.min()):.4f}")
    assert nbad == 0, f"{tag}: {nbad} elements beyond the gate, worst ratio {worst:.3f}"
    if clamp:
        assert int(torch.count_nonzero(got[(x < 0) | (x > Rr)])) == 0, f"{tag}: gradient where the clamp is active"
    # outside [H, W]: bit-unchanged
    assert torch.equal(g0.view(torch.int32)[~inside], torch.full((B, Cn, rows, rs), nan).view(torch.int32)[~inside]), tag
    # value and per-channel MS-SSIM
    assert abs(float(l0) - float(want_loss)) <= 1e-6 * abs(float(want_loss)), (tag, float(l0), float(want_loss))
    perr = float(((p0.view(B, Cn) - want_M).abs() / want_M).max())
    print(f"{tag}: per_channel_out, largest relative error {perr:.3e}")
    assert perr <= 1e-12, (tag, perr)
    # two runs, and a run on poisoned scratch: bit-identical
    for poison in (False, True):
        g1, l1, p1 = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W, poison))
        assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)) and torch.equal(l1, l0) and torch.equal(p1, p0), (tag, poison)
    # value only (gx_add = NULL): the same value, the same per-channel numbers
    _, lv, pv = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W), with_grad=False)
    assert torch.equal(lv, l0) and torch.equal(pv, p0), tag
    # a prefilled destination is added to, in the gradient and (accumulate = 1) in the value
    g2, l2, _ = run(noise, 2.5, 1, _scratch(lib, B, Cn, H, W))
    nbad, worst = _gate(g2[..., :H, :W].double(), want, prefill=noise.double())
    assert nbad == 0, f"{tag}: {nbad} elements of the prefilled destination beyond the gate, worst ratio {worst:.3f}"
    assert torch.equal(g2[..., :H, :W], noise + g0[..., :H, :W]), tag          # (the same fp32 add)
    assert torch.equal(l2, torch.tensor([2.5]) + l0), (tag, float(l2), float(l0))


# ------------------------------------------------------------------ 2. the pyramid and the gradient levels in the scratch
@pytest.mark.parametrize("idx,clamp,Rr", [(0, 1, 255.0), (2, 1, 1.0), (2, 0, 255.0)], ids=["odd-chain", "mixed-parity", "no-clamp"])
def test_device_pyramid_equals_the_reference_pyramid_bit_for_bit(idx, clamp, Rr):
    """Levels 1 .. 4 of both pyramids read from the scratch (un-normalised: pooled clamp(x), pooled y) against the restatement's
    pooling of the same fp32 values widened: the same bits.  The fp64 gradient levels next to them against the reference's."""
    _lib, lib = _lib_()
    shape = CASES[idx][0]
    B, Cn, H, W = shape
    x, y, scale, _, _, _, want_levels = _case(idx, clamp, Rr)
    scratch = _scratch(lib, B, Cn, H, W, poison=True)
    gx, loss = torch.zeros(shape, device="cuda"), torch.zeros(1, device="cuda")
    xd, yd = x.cuda(), y.cuda()
    _lib.check(lib.m2t_msssim_loss_tensor(_lib.ptr(xd), _lib.ptr(yd), B, Cn, H, W, Cn * H * W, W, Rr, clamp, scale, _lib.ptr(gx),
                                          _lib.ptr(loss), None, 0, _lib.ptr(scratch), _lib.stream_ptr()), "m2t_msssim_loss_tensor")
    torch.cuda.synchronize()
    words = scratch.cpu().view(torch.float64)
    xs = R.pyramid(x.double().clamp(0.0, Rr) if clamp else x.double())
    ys = R.pyramid(y.double())
    for l in range(1, R.LEVELS):
        h, w = xs[l].shape[-2:]
        for region, want in ((2, xs[l]), (3, ys[l])):
            off = lib.m2t_msssim_loss_scratch_offset(B, Cn, H, W, region, l)
            got = words[off // 8: off // 8 + B * Cn * h * w].view(B, Cn, h, w)
            assert torch.equal(got.view(torch.int64), want.contiguous().view(torch.int64)), (shape, "x" if region == 2 else "y", l)
        off = lib.m2t_msssim_loss_scratch_offset(B, Cn, H, W, 4, l)
        got = words[off // 8: off // 8 + B * Cn * h * w].view(B, Cn, h, w)
        ref = want_levels[l - 1]
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"{shape} level {l} ({h} x {w}): gradient level, {err:.3e} of its largest entry")
        assert err <= 1e-11, (shape, l, err)


# ------------------------------------------------------------------ 3. the zero rule
def test_zero_rule_leaves_the_destination_untouched():
    """x = 1 - y: every (image, channel) has negative level means, M = 0: a prefilled gx_add keeps its bits (-0.0 and NaN included)
    and the loss grows by scale * B * C.  Then one dead channel next to two live ones: only the dead one is left alone."""
    _lib, lib = _lib_()
    shape = (2, 3, 176, 176)
    B, Cn, H, W = shape
    _, y = R.smooth_pair(shape, 0.0, seed=4)
    x = (1.0 - y).contiguous()
    _, _, want_M, _ = R.value_and_grad(x, y)
    assert int(torch.count_nonzero(want_M)) == 0
    scale = 0.25
    g = torch.Generator().manual_seed(5)
    prefill = torch.randn(shape, generator=g)
    prefill[0, 0, 0, :4] = torch.tensor([-0.0, 0.0, float("nan"), float("inf")])
    gx, loss = prefill.cuda(), torch.full((1,), 1.5, device="cuda")
    per = torch.full((B * Cn,), float("nan"), dtype=torch.float64, device="cuda")

    yd, scratch = y.cuda(), _scratch(lib, B, Cn, H, W, True)

    def call(xd, clamp):
        _lib.check(lib.m2t_msssim_loss_tensor(_lib.ptr(xd), _lib.ptr(yd), B, Cn, H, W, Cn * H * W, W, 1.0, clamp, scale, _lib.ptr(gx),
                                              _lib.ptr(loss), _lib.ptr(per), 1, _lib.ptr(scratch), _lib.stream_ptr()),
                   "m2t_msssim_loss_tensor")
        torch.cuda.synchronize()

    call(x.cuda(), 1)
    assert torch.equal(gx.cpu().view(torch.int32), prefill.view(torch.int32))
    assert torch.equal(loss.cpu(), torch.tensor([1.5]) + torch.tensor([scale * B * Cn], dtype=torch.float32))
    assert torch.equal(per.cpu(), torch.zeros(B * Cn, dtype=torch.float64))
    # channel 0 of image 1 dead, the rest alive
    xm = (y * 0.9 + 0.02).contiguous()
    xm[1, 0] = x[1, 0]
    _, want, want_M, _ = R.value_and_grad(xm, y, 1.0, False, scale)
    assert float(want_M[1, 0]) == 0.0 and int(torch.count_nonzero(want_M)) == B * Cn - 1
    prefill = torch.randn(shape, generator=g) * float(want.abs().max())
    gx.copy_(prefill)
    call(xm.cuda(), 0)
    got = gx.cpu()
    assert torch.equal(got[1, 0].view(torch.int32), prefill[1, 0].view(torch.int32))
    live = torch.ones(B, Cn, dtype=torch.bool)
    live[1, 0] = False
    assert float((got[live] != prefill[live]).double().mean()) > 0.5
    nbad, worst = _gate(got.double(), want, prefill=prefill.double())
    assert nbad == 0, (nbad, worst)
    assert float(((per.cpu().view(B, Cn) - want_M).abs() / want_M.clamp(min=1e-300))[live].max()) <= 1e-12


# ------------------------------------------------------------------ 4. the plan entry
def _srpre(plan, B, scale):
    Hp, Wp = plan.query("padded_h") * scale, plan.query("padded_w") * scale
    return plan.ws_tensor("srpre", dtype=torch.float32).view(B, 3, Hp, Wp)


def _hr_for(pre, Hs, Ws, seed=0):
    """The target for a pre-clamp output read back from the workspace: HR = clamp(clamp(pre) + 0.05 randn)."""
    g = torch.Generator().manual_seed(100 + seed)
    inner = pre[..., :Hs, :Ws].float().cpu().clamp(0.0, 1.0)
    return (inner + 0.05 * torch.randn(inner.shape, generator=g)).clamp(0.0, 1.0).contiguous().cuda()


_PAIRS = {}


def _pair(scale, dtype, B, H, W, step=0):
    """(x, hr) for a model of this kind: hr is built from what an untrained twin gives for x (computed once per key)."""
    key = (scale, dtype, B, H, W, step)
    if key not in _PAIRS:
        _lib, lib = _lib_()
        model = _model(scale, dtype, NB)
        x, _ = _images(B, H, W, scale, step)
        plan = model._plan_for(x)
        _forward(lib, model, plan, x)
        torch.cuda.synchronize()
        _PAIRS[key] = (x, _hr_for(_srpre(plan, B, scale), H * scale, W * scale, step))
    return _PAIRS[key]


def _pixel(lib, plan, hr, out, weight=1.0, divisor=None, deferred=False):
    from m2trans_amd import _lib
    fn = lib.m2t_pixel_loss_deferred if deferred else lib.m2t_pixel_loss
    return fn(plan.handle, 0, 0.0, _lib.ptr(hr), weight, float(hr.numel() if divisor is None else divisor), 1.0, _lib.ptr(out),
              _lib.ptr(plan.workspace), _lib.stream_ptr())


def _msssim(lib, plan, hr, out, weight=LAM, divisor=None, accumulate=0, scratch=None):
    from m2trans_amd import _lib
    if scratch is None:
        scratch = _scratch(lib, hr.shape[0], 3, hr.shape[-2], hr.shape[-1])
    rc = lib.m2t_msssim_loss(plan.handle, _lib.ptr(hr), weight, float(hr.shape[0] * 3 if divisor is None else divisor), 1.0, _lib.ptr(out),
                             accumulate, _lib.ptr(scratch), _lib.ptr(plan.workspace), _lib.stream_ptr())
    torch.cuda.synchronize()             # (the scratch of this helper dies with the call)
    return rc


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("scale,shape", [(4, (1, 44, 48)), (3, (1, 54, 64)), (2, (1, 88, 96))], ids=["x4-176x192", "x3-162x192", "x2-176x192"])
def test_plan_entry_adds_the_seed_against_fp64(dtype, scale, shape):
    """m2t_pixel_loss(weight 0) then m2t_msssim_loss: ws:gpre against the restatement on the read-back bits of ws:srpre; then with the
    L1 weight 1 the sum of both references (the L1 seed being sign(d) * (float)(1 / N), include/m2t.h)."""
    _lib, lib = _lib_()
    B, H, W = shape
    model = _model(scale, dtype, NB)
    x, _ = _images(B, H, W, scale)
    plan = model._plan_for(x)
    _forward(lib, model, plan, x)
    torch.cuda.synchronize()
    pre = _srpre(plan, B, scale).clone()
    Hs, Ws = H * scale, W * scale
    hr = _hr_for(pre, Hs, Ws)
    assert tuple(pre.shape[-2:]) != (Hs, Ws), "the shapes are meant to be reflect-padded"
    pad = torch.ones(pre.shape, dtype=torch.bool)
    pad[..., :Hs, :Ws] = False
    clamped = ((pre < 0) | (pre > 1)).cpu()
    tag = f"{dtype} x{scale} {shape}"
    inner = pre[..., :Hs, :Ws].cpu()
    share = {"below 0": float((inner < 0).double().mean()), "above 1": float((inner > 1).double().mean()),
             "inside": float(((inner >= 0) & (inner <= 1)).double().mean())}
    assert share["below 0"] >= 0.05 and share["above 1"] >= 0.03 and share["inside"] >= 0.25, f"{tag}: coverage {share}"
    want_loss, want = R.loss_and_seed(pre.cpu(), hr.cpu(), weight=LAM)
    _, _, want_M, _ = R.value_and_grad(pre[..., :Hs, :Ws].cpu(), hr.cpu(), 1.0, True)
    assert bool((want_M > 0).all()), (tag, want_M)
    l1, out = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    # the multi-scale term alone
    gpre.fill_(float("nan"))
    assert _pixel(lib, plan, hr, l1, weight=0.0) == 0 and _msssim(lib, plan, hr, out) == 0
    got = gpre.view(pre.shape).double().cpu()
    assert bool(torch.isfinite(got).all()), tag
    assert int(torch.count_nonzero(got[pad])) == 0, f"{tag}: seed in the padding"
    assert int(torch.count_nonzero(got[clamped])) == 0, f"{tag}: seed where the clamp is active"
    assert int(torch.count_nonzero(want)) > 0.2 * hr.numel()
    nbad, worst = _gate(got[..., :Hs, :Ws], want[..., :Hs, :Ws])
    print(f"{tag}: MS-SSIM seed, largest |got - ref| / bound {worst:.3f}; value {float(out):.9e} against {float(want_loss):.9e}; "
          f"min M {float(want_M.min()):.4f}")
    assert nbad == 0, f"{tag}: {nbad} seed elements beyond the gate, worst ratio {worst:.3f}"
    assert abs(float(out) - float(want_loss)) <= 1e-6 * abs(float(want_loss)), (tag, float(out), float(want_loss))
    # behind the L1 seed
    gpre.fill_(float("nan"))
    assert _pixel(lib, plan, hr, l1, weight=1.0) == 0 and _msssim(lib, plan, hr, out) == 0
    got = gpre.view(pre.shape).double().cpu()
    inner = pre[..., :Hs, :Ws].double().cpu()
    d = inner.clamp(0.0, 1.0) - hr.double().cpu()
    seed_l1 = RP.derivative("l1", d) * RP.clamp_mask(inner) * float(torch.tensor(1.0 / hr.numel(), dtype=torch.float32))
    nbad, worst = _gate(got[..., :Hs, :Ws], want[..., :Hs, :Ws], prefill=seed_l1)
    assert nbad == 0, f"{tag}: {nbad} elements of L1 + MS-SSIM beyond the gate, worst ratio {worst:.3f}"
    assert int(torch.count_nonzero(got[pad])) == 0 and int(torch.count_nonzero(got[clamped])) == 0, tag


def test_plan_entry_state_and_argument_errors():
    """State rules of m2t_ssim_loss; an SR side <= 160 is refused before any launch."""
    _lib, lib = _lib_()
    model = _model(4, "fp32", NB)
    x, hr = _pair(4, "fp32", 1, 44, 48)
    plan = model._plan_for(x)
    out = torch.zeros(1, device="cuda")
    assert _msssim(lib, plan, hr, out) == STATE                      # before a forward
    _forward(lib, model, plan, x)
    assert _msssim(lib, plan, hr, out) == STATE                      # before any seed
    assert _pixel(lib, plan, hr, out, deferred=True) == 0
    assert _msssim(lib, plan, hr, out) == STATE                      # a deferred request leaves no materialised seed
    assert b"materialised" in lib.m2t_last_error_string()
    assert _pixel(lib, plan, hr, out) == 0
    assert _msssim(lib, plan, hr, out) == 0
    scratch = _scratch(lib, 1, 3, 176, 192)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    for bad in (dict(hr=None), dict(out=None), dict(scratch=None), dict(ws=None), dict(R=0.0), dict(div=0.0), dict(div=float("nan"))):
        a = dict(hr=_lib.ptr(hr), out=_lib.ptr(out), scratch=_lib.ptr(scratch), ws=ws, R=1.0, div=3.0)
        a.update(bad)
        assert lib.m2t_msssim_loss(plan.handle, a["hr"], LAM, a["div"], a["R"], a["out"], 0, a["scratch"], a["ws"], st) == ARG, bad
    torch.cuda.synchronize()
    # 40 x 56 at x4: an SR image of 160 x 224
    xs, hs = _images(1, 40, 56, 4)
    small = model._plan_for(xs)
    _forward(lib, model, small, xs)
    assert _pixel(lib, small, hs, out) == 0
    seed = small.ws_tensor("gpre", dtype=torch.float32).clone()
    assert lib.m2t_msssim_loss(small.handle, _lib.ptr(hs), LAM, 3.0, 1.0, _lib.ptr(out), 0, _lib.ptr(scratch), _lib.ptr(small.workspace), st) == ARG
    assert b"larger than 160" in lib.m2t_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(small.ws_tensor("gpre", dtype=torch.float32), seed)
    assert lib.m2t_msssim_loss_scratch_bytes(1, 3, 160, 224) == 0


# ------------------------------------------------------------------ 5. TrainStep against the sequence by hand and against autograd
def _by_hand(model, plan, x, hr, lam=LAM, pix_div=None, ms_div=None):
    """(l1 [1], msssim [1], gradients): m2t_forward -> m2t_pixel_loss (l1) -> m2t_msssim_loss -> m2t_backward into fresh buffers."""
    _lib, lib = _lib_()
    l1, ms = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    grads = torch.full_like(model.flat_params, float("nan"))
    _forward(lib, model, plan, x)
    assert _pixel(lib, plan, hr, l1, divisor=pix_div) == 0
    assert _msssim(lib, plan, hr, ms, weight=lam, divisor=ms_div) == 0
    _backward(lib, model, plan, x, grads)
    torch.cuda.synchronize()
    return l1, ms, grads


@pytest.mark.parametrize("dtype,scale,shape,tol", [("bf16", 4, (2, 44, 48), 1e-2), ("fp32", 2, (2, 88, 96), 1e-5)])
def test_train_step_is_the_sequence_by_hand_and_matches_the_autograd_route(dtype, scale, shape, tol):
    """Two steps with different batches: loss, gradients, parameters and moments bit-identical to m2t_forward -> m2t_pixel_loss ->
    m2t_msssim_loss -> m2t_backward -> m2t_adam_step on a twin.  The first step's gradients are also compared with the route a user
    had to take: sr = model(x), torch's L1 plus the fp32 torch form of the restatement, backward() -- rel-L2 1e-5 in fp32, 1e-2 in
    bf16, the gates of the SSIM term's test of the same name."""
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    B, H, W = shape
    m_a, m_b = _model(scale, dtype, NB), _model(scale, dtype, NB)
    ts = TrainStep(m_a, lr=1e-4, world_size=1, lambda_msssim=LAM)
    exp_avg, exp_avg_sq = torch.zeros_like(m_b.flat_params), torch.zeros_like(m_b.flat_params)
    first_grads = None
    for step in range(2):
        x, hr = _pair(scale, dtype, B, H, W, step)
        loss = ts.step(x, hr)
        torch.cuda.synchronize()
        plan = m_b._plan_for(x)
        l1, ms, grads = _by_hand(m_b, plan, x, hr)
        if step == 0:
            first_grads = grads.clone()
        n = grads.numel()
        _lib.check(lib.m2t_adam_step(_lib.ptr(m_b.flat_params), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), n, 1e-4, 0.9,
                                     0.999, 1e-8, step + 1, 1.0, _lib.stream_ptr()), "m2t_adam_step")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(grads).all()) and 0 < float(ms) < LAM and float(l1) > 0
        assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.msssim_loss, ms) and torch.equal(loss, l1 + ms), (step, float(loss))
        assert ts.loss is loss
        assert_flat_equal(m_a, ts.grads, grads, f"gradients, step {step}")
        assert_flat_equal(m_a, m_a.flat_params.detach(), m_b.flat_params.detach(), f"parameters, step {step}")
        assert_flat_equal(m_a, ts.exp_avg, exp_avg, f"exp_avg, step {step}")
        assert_flat_equal(m_a, ts.exp_avg_sq, exp_avg_sq, f"exp_avg_sq, step {step}")
    # the autograd route, on the weights of step 0
    model = _model(scale, dtype, NB)
    x, hr = _pair(scale, dtype, B, H, W, 0)
    sr = model(x)
    M = R.ms_ssim(sr, hr)
    assert bool((M > 0).all()), M
    want_loss = torch.nn.L1Loss()(sr, hr) + LAM * (1.0 - M).mean()
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
    assert float(want.norm()) > 0 and bool(torch.isfinite(want).all())
    err = float((got - want).norm() / want.norm())
    print(f"{dtype} x{scale}: by-hand gradients against the autograd route, rel-L2 {err:.3e} (gate {tol:g})")
    assert err <= tol, (dtype, err)
    # the term is live: the L1 step alone gives other gradients
    ts0 = TrainStep(_model(scale, dtype, NB), world_size=1)
    ts0.forward_backward(x, hr)
    torch.cuda.synchronize()
    assert not torch.equal(ts0.grads, first_grads)


# ------------------------------------------------------------------ 6. the default step is untouched
def test_lambda_msssim_zero_is_the_default_step_bit_for_bit():
    from m2trans_amd.train_step import TrainStep
    scale, dtype, B, H, W = 4, "bf16", 2, 44, 48
    res = []
    for kw in ({}, {"lambda_msssim": 0.0}):
        model = _model(scale, dtype, NB)
        ts = TrainStep(model, lr=1e-4, world_size=1, **kw)
        assert ts.msssim_loss is None and ts._msssim_scratch == {}
        out = []
        for step in range(2):
            x, hr = _pair(scale, dtype, B, H, W, step)
            loss = ts.step(x, hr)
            torch.cuda.synchronize()
            assert ts.msssim_loss is None and loss is ts.l1_loss and ts._msssim_scratch == {}
            out.append((loss.clone(), ts.grads.clone(), model.flat_params.detach().clone()))
        res.append((model, out))
    (model, a), (_, b) = res
    for step in range(2):
        assert torch.equal(a[step][0], b[step][0])
        assert_flat_equal(model, a[step][1], b[step][1], f"gradients, step {step}")
        assert_flat_equal(model, a[step][2], b[step][2], f"parameters, step {step}")
    # with the term on, an SR image of 160 x 224 is refused by the step itself, on the host
    from m2trans_amd._lib import M2TError
    with pytest.raises(M2TError, match="larger than 160"):
        TrainStep(_model(scale, dtype, NB), world_size=1, lambda_msssim=LAM).forward_backward(*_images(1, 40, 56, scale))


# ------------------------------------------------------------------ 7. accumulation
def test_accumulated_msssim_equals_the_micro_batch_gradients_summed_in_call_order():
    """accum_steps = 2 at micro-batch (1, 44, 48), bf16 x4: the accumulated buffer is the fp32 sum, in call order, of the two
    micro-batch gradients taken by hand with the cycle's divisors; ts.msssim_loss is the sum of the two values."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    x, hr = _pair(4, "bf16", 2, 44, 48)
    m_a, m_b = _model(4, "bf16", NB), _model(4, "bf16", NB)
    ts = TrainStep(m_a, world_size=1, accum_steps=2, lambda_msssim=LAM)
    ts.forward_backward(x[0:1], hr[0:1])
    with pytest.raises(M2TError):
        ts.optimizer_step()                                          # in mid-cycle
    with pytest.raises(M2TError):
        ts.set_lambda_msssim(0.0)
    loss = ts.forward_backward(x[1:2], hr[1:2])
    torch.cuda.synchronize()
    parts = []
    for i in range(2):
        cx, chr_ = x[i:i + 1].contiguous(), hr[i:i + 1].contiguous()
        parts.append(_by_hand(m_b, m_b._plan_for(cx), cx, chr_, pix_div=hr.numel(), ms_div=2 * 3))
    assert float(parts[1][2].abs().max()) > 0 and float(parts[1][1]) > 0
    assert torch.equal(ts.msssim_loss, parts[0][1] + parts[1][1]), (float(ts.msssim_loss), float(parts[0][1] + parts[1][1]))
    assert torch.equal(ts.l1_loss, parts[0][0] + parts[1][0])
    assert torch.equal(loss, ts.l1_loss + ts.msssim_loss)
    assert_flat_equal(m_a, ts.grads, parts[0][2] + parts[1][2], "accumulated L1 + MS-SSIM")
    ts.optimizer_step()
    assert ts.micro_count == 0


# ------------------------------------------------------------------ 8. the three optional terms together
def test_ssim_msssim_and_fft_terms_add_their_seeds():
    """TrainStep(lambda_ssim, lambda_msssim, lambda_fft) issues pixel -> SSIM -> MS-SSIM -> FFT -> backward: bit-identical to that
    sequence by hand; and the seed after the four contributions against the four taken alone: three fp32 adds, each within half an ulp
    of its partial sum -> 2e-7 (|a| + |b| + |c| + |d|) per element.  48 x 48 at x4: 192 x 192 suits the transform (2^6 * 3)."""
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    scale, dtype, B, H, W = 4, "bf16", 1, 48, 48
    x, hr = _pair(scale, dtype, B, H, W)
    Hs = Ws = 192
    lam_s, lam_f = 0.1, 0.05
    m_a, m_b = _model(scale, dtype, NB), _model(scale, dtype, NB)
    ts = TrainStep(m_a, world_size=1, lambda_ssim=lam_s, lambda_msssim=LAM, lambda_fft=lam_f)
    loss = ts.forward_backward(x, hr)
    torch.cuda.synchronize()
    plan = m_b._plan_for(x)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    l1, ss, ms, ff = (torch.full((1,), float("nan"), device="cuda") for _ in range(4))
    s_ssim = torch.empty(lib.m2t_ssim_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    s_fft = torch.empty(lib.m2t_fft_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    _forward(lib, m_b, plan, x)

    def seed(pixel_weight, with_ssim, with_ms, with_fft):
        assert _pixel(lib, plan, hr, l1, weight=pixel_weight) == 0
        if with_ssim:
            _lib.check(lib.m2t_ssim_loss(plan.handle, _lib.ptr(hr), lam_s, float(B * 3 * (Hs - 10) * (Ws - 10)), 1.0, _lib.ptr(ss), 0,
                                         _lib.ptr(s_ssim), ws, st), "m2t_ssim_loss")
        if with_ms:
            assert _msssim(lib, plan, hr, ms) == 0
        if with_fft:
            _lib.check(lib.m2t_fft_loss(plan.handle, _lib.ptr(hr), lam_f, float(B * 3 * Hs * (Ws // 2 + 1) * 2), 1.0, 0, _lib.ptr(ff), 0,
                                        _lib.ptr(s_fft), ws, st), "m2t_fft_loss")
        torch.cuda.synchronize()
        return gpre.clone()

    parts = [seed(1.0, False, False, False), seed(0.0, True, False, False), seed(0.0, False, True, False), seed(0.0, False, False, True)]
    for t in parts:
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
    full = seed(1.0, True, True, True).double().cpu()
    parts = [t.double().cpu() for t in parts]
    excess = (full - sum(parts)).abs() - 2e-7 * sum(t.abs() for t in parts)
    assert float(excess.max()) <= 0.0, float(excess.max())
    g_b = torch.full_like(m_b.flat_params, float("nan"))
    _backward(lib, m_b, plan, x, g_b)
    torch.cuda.synchronize()
    assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.ssim_loss, ss) and torch.equal(ts.msssim_loss, ms) and torch.equal(ts.fft_loss, ff)
    assert torch.equal(loss, ts.l1_loss + ts.ssim_loss + ts.msssim_loss + ts.fft_loss)
    assert_flat_equal(m_a, ts.grads, g_b, "pixel + SSIM + MS-SSIM + FFT")


# ------------------------------------------------------------------ 9. the autograd Function and the metric
def test_ms_ssim_loss_function_and_metric():
    from m2trans_amd.losses import MSSSIMLoss, ms_ssim_loss
    from m2trans_amd.metrics import ms_ssim_device
    shape = (2, 3, 176, 192)
    x, y = R.smooth_pair(shape, 0.1, seed=21)
    leaf64 = x.double().requires_grad_(True)
    M = R.ms_ssim(leaf64, y.double())
    want = (1.0 - M).mean()
    want.backward()
    leaf = x.cuda().requires_grad_(True)
    got = ms_ssim_loss(leaf, y.cuda())
    (got * 3.0).backward()                                          # (an upstream factor reaches the gradient)
    torch.cuda.synchronize()
    assert got.shape == () and abs(float(got.detach()) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))
    nbad, worst = _gate(leaf.grad.double().cpu() / 3.0, leaf64.grad)
    print(f"ms_ssim_loss Function: largest |got - ref| / bound {worst:.3f}")
    # (the division by 3 undoes an fp32 product: one more rounding on each side of it, 1.2e-7 |ref| -- inside the 1e-6 |ref| term)
    assert nbad == 0, (nbad, worst)
    assert float(MSSSIMLoss()(x.cuda(), y.cuda())) == float(got)
    m = ms_ssim_device(x.cuda(), y.cuda())
    assert m.dtype == torch.float64 and tuple(m.shape) == (2,)
    assert float(((m.cpu() - M.detach().mean(dim=1)).abs() / M.detach().mean(dim=1)).max()) <= 1e-12
    m255 = ms_ssim_device(x.cuda() * 255.0, y.cuda() * 255.0, data_range=255.0)
    assert float((m255.cpu() - m.cpu()).abs().max()) <= 1e-6          # (x * 255 rounds in fp32: another input, the same image)
