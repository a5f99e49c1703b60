"""-m gpu: the VIF loss term (k_vif_loss.hip; m2t_vif_loss_tensor, m2t_vif_loss, losses.vif_loss, metrics.vif_device,
TrainStep(lambda_vif=...)) against the fp64 restatement tests/vif_loss_ref.py: the plan-free entry per element, the pyramid levels read
back from the scratch, the flat image, the plan entry on the forward's own pre-clamp output, TrainStep against the sequence composed by
hand and against the autograd route, the default step, accumulation, and the four optional terms together.

The gate of a gradient element is |got - ref| <= 1e-6 |ref| + 1e-7 max_b |ref| + 6e-8 |prefill + ref|, the form the MS-SSIM test
derives: everything between the fp32 inputs and the single fp32 rounding is fp64, so what remains is the order of the fp64 sums and one
rounding (6e-8), plus -- where the destination held something -- half an ulp of the sum.  VIF adds the cancellation of G*(u u) - mx^2
on the 0 .. 255 scale (an absolute 1e-11 on a against sigma_n_sq = 2); the host emulation of the kernel text, in the kernel's own sum
order (tests/test_vif_loss_cpu.py), stays within 0.05 of the first two terms, so they stand as they are.

Inputs: the "mixed" family of tests/vif_loss_ref.py wherever the plan-free gradient is compared -- y smoothed noise with an exactly
constant patch (dead entries), x = 0.5 y on the left columns (sv_raw ~ 0.25 EPS: the clamped branch), x = y + sigma randn elsewhere
(the open branch, a share of it outside [0, R]); the three shares at scale 0 are asserted non-zero through the restatement before
anything is compared.  x = y is never used where a gradient is compared.  In the plan and TrainStep tests SR is what the model gives,
and HR = clamp(clamp(pre) + 0.05 randn) is built from the read-back pre-clamp output."""
import pytest
import torch

from tests import pixel_loss_ref as RP
from tests import vif_loss_ref as V
from tests.gpu_util import assert_flat_equal
from tests.test_gpu_msssim_loss import _hr_for, _model, _pair, _pixel, _srpre
from tests.test_gpu_pixel_loss import _backward, _forward, _images

pytestmark = pytest.mark.gpu

ARG, STATE = -2, -3
LAM = 0.1
NB = 1
N0 = 2.0                 # sigma_n_sq, the library's default
HALF_ULP = 6e-8          # 2^-24 = 5.96e-8


def _lib_():
    from m2trans_amd import _lib
    return _lib, _lib.load()


def _scratch(lib, B, Cn, H, W, poison=False):
    n = lib.m2t_vif_loss_scratch_bytes(B, Cn, H, W)
    assert n > 0
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    if poison:
        t.fill_(0xFF)
    return t


def _gate(got, ref, prefill=None):
    """(elements beyond the gate, largest |got - want| / bound) for [B,C,H,W] fp64 tensors; max_b is taken per image."""
    top = ref.abs().amax(dim=(-3, -2, -1), keepdim=True)
    want = ref if prefill is None else prefill + ref
    bound = 1e-6 * ref.abs() + 1e-7 * top + HALF_ULP * want.abs()
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), (err > 0).double() * float("inf"))
    return int((err > bound).sum()), float(ratio.max())


# ------------------------------------------------------------------ 1. the plan-free entry against fp64
# (shape, (rows, row stride) of the buffer that holds x or None = contiguous)
CASES = [((1, 1, 41, 41), None),                        # the smallest: maps of 25, 9, 3 and 1 entries a side
         ((2, 3, 42, 57), (45, 64)),                    # strided x in a NaN-filled buffer: row stride 64, image stride 3 * 45 * 64
         ((1, 3, 48, 61), None),
         ((1, 1, 64, 300), None)]                       # levels 300 / 146 / 71 / 35 wide: several tiles at every scale
CASE_IDS = ["41", "strided", "48x61", "wide"]
_REF = {}


def _case(idx, clamp, Rr, nn=N0):
    """Inputs and the reference of one case, computed once and shared (never modified)."""
    key = (idx, clamp, Rr, nn)
    if key not in _REF:
        shape = CASES[idx][0]
        x, y = V.mixed_pair(shape, seed=10 + idx, R=Rr)
        scale = 0.37 / shape[0]
        loss, grad, vif, shares = V.value_and_grad(x, y, Rr, bool(clamp), scale, nn)
        assert min(shares[0].values()) > 0, (shape, shares[0])          # dead, clamped and open entries at scale 0
        assert int(((x < 0) | (x > Rr)).sum()) > 0
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0, shape
        _REF[key] = (x, y, scale, loss, grad, vif, shares)
    return _REF[key]


# every shape with clamp 0 / 1 and R 1 / 255 at the default sigma_n_sq, and a non-default sigma_n_sq once
RUNS = [(i, c, r, N0) for i in range(len(CASES)) for c in (0, 1) for r in (1.0, 255.0)] + [(2, 1, 1.0, 0.7)]


@pytest.mark.parametrize("idx,clamp,Rr,nn", RUNS, ids=[f"{CASE_IDS[i]}-clamp{c}-R{r:g}-n{n:g}" for i, c, r, n in RUNS])
def test_plan_free_entry_against_fp64(idx, clamp, Rr, nn):
    _lib, lib = _lib_()
    shape, layout = CASES[idx]
    B, Cn, H, W = shape
    x, y, scale, want_loss, want, want_v, shares = _case(idx, clamp, Rr, nn)
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
        per = torch.full((B,), nan, dtype=torch.float64, device="cuda")
        rc = lib.m2t_vif_loss_tensor(_lib.ptr(xbuf), _lib.ptr(yd), B, Cn, H, W, Cn * rows * rs, rs, Rr, nn, clamp, scale,
                                     _lib.ptr(gbuf) if with_grad else None, _lib.ptr(loss), _lib.ptr(per), accumulate,
                                     _lib.ptr(scratch), _lib.stream_ptr())
        _lib.check(rc, "m2t_vif_loss_tensor")
        torch.cuda.synchronize()
        return gbuf.cpu(), loss.cpu(), per.cpu()

    tag = f"{shape} clamp {clamp} R {Rr:g} n {nn:g}"
    g0, l0, p0 = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W))
    got = g0[..., :H, :W].double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(l0).all()), tag
    nbad, worst = _gate(got, want)
    print(f"{tag}: gradient, largest |got - ref| / bound {worst:.3f} (max |ref| {float(want.abs().max()):.3e}); "
          f"value {float(l0):.9e} against {float(want_loss):.9e}; VIF {want_v.tolist()}; shares at scale 0 {shares[0]}")
    assert nbad == 0, f"{tag}: {nbad} elements beyond the gate, worst ratio {worst:.3f}"
    if clamp:
        assert int(torch.count_nonzero(got[(x < 0) | (x > Rr)])) == 0, f"{tag}: gradient where the clamp is active"
    # outside [H, W]: bit-unchanged
    assert torch.equal(g0.view(torch.int32)[~inside], torch.full((B, Cn, rows, rs), nan).view(torch.int32)[~inside]), tag
    # value (within fp32 rounding) and per-image VIF
    assert abs(float(l0) - float(want_loss)) <= 1.2e-7 * abs(float(want_loss)), (tag, float(l0), float(want_loss))
    perr = float(((p0 - want_v).abs() / want_v).max())
    print(f"{tag}: per_image_out, largest relative error {perr:.3e}")
    assert perr <= 1e-12, (tag, perr)
    # two runs, and a run on poisoned scratch: bit-identical
    for poison in (False, True):
        g1, l1, p1 = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W, poison))
        assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)) and torch.equal(l1, l0) and torch.equal(p1, p0), (tag, poison)
    # value only (gx_add = NULL): the same value, the same per-image numbers; a NaN-prefilled destination is not needed for it
    _, lv, pv = run(nan, nan, 0, _scratch(lib, B, Cn, H, W), with_grad=False)
    assert torch.equal(lv, l0) and torch.equal(pv, p0), tag
    # a prefilled destination is added to, in the gradient and (accumulate = 1) in the value
    g2, l2, _ = run(noise, 2.5, 1, _scratch(lib, B, Cn, H, W))
    nbad, worst = _gate(g2[..., :H, :W].double(), want, prefill=noise.double())
    assert nbad == 0, f"{tag}: {nbad} elements of the prefilled destination beyond the gate, worst ratio {worst:.3f}"
    assert torch.equal(g2[..., :H, :W], noise + g0[..., :H, :W]), tag          # (the same fp32 add)
    assert torch.equal(l2, torch.tensor([2.5]) + l0), (tag, float(l2), float(l0))
    # a NaN-prefilled destination stays NaN where it is added to and untouched (NaN as well) elsewhere: nothing is overwritten
    g3, _, _ = run(nan, nan, 0, _scratch(lib, B, Cn, H, W))
    assert bool(torch.isnan(g3).all()), tag


# ------------------------------------------------------------------ 2. the pyramid and the gradient levels in the scratch
@pytest.mark.parametrize("idx,clamp,Rr", [(0, 1, 255.0), (1, 1, 1.0), (3, 0, 255.0)], ids=["41", "rgb-two-images", "wide-no-clamp"])
def test_device_pyramid_levels_against_the_restatement(idx, clamp, Rr):
    """Levels 1 .. 3 of both pyramids read from the scratch through m2t_vif_loss_scratch_offset: within 1e-12 (relative to the level's
    largest entry) of the restatement; the fp64 gradient levels next to them within 1e-10; the record holds sum t, sum d, VIF."""
    _lib, lib = _lib_()
    shape = CASES[idx][0]
    B, Cn, H, W = shape
    x, y, scale, _, _, want_v, _ = _case(idx, clamp, Rr)
    scratch = _scratch(lib, B, Cn, H, W, poison=True)
    gx, loss = torch.zeros(shape, device="cuda"), torch.zeros(1, device="cuda")
    xd, yd = x.cuda(), y.cuda()
    _lib.check(lib.m2t_vif_loss_tensor(_lib.ptr(xd), _lib.ptr(yd), B, Cn, H, W, Cn * H * W, W, Rr, N0, clamp, scale, _lib.ptr(gx),
                                       _lib.ptr(loss), None, 0, _lib.ptr(scratch), _lib.stream_ptr()), "m2t_vif_loss_tensor")
    torch.cuda.synchronize()
    words = scratch.cpu().view(torch.float64)
    v, den, us, vs, G, _ = V.details(x, y, Rr, bool(clamp), N0)
    for s in range(1, V.SCALES):
        h, w = us[s].shape[-2:]
        for region, want, tol in ((2, us[s], 1e-12), (3, vs[s], 1e-12), (4, G[s], 1e-10)):
            off = lib.m2t_vif_loss_scratch_offset(B, Cn, H, W, region, s)
            got = words[off // 8: off // 8 + B * h * w].view(B, h, w)
            top = float(want.abs().max())           # (at 41 x 41 the one map entry of scale 3 may be dead: an all-zero level)
            err = float((got - want).abs().max()) / top if top > 0 else float(got.abs().max())
            print(f"{shape} region {region} level {s} ({h} x {w}): {err:.3e} of its largest entry")
            assert err <= tol, (shape, region, s, err)
    rec = words[lib.m2t_vif_loss_scratch_offset(B, Cn, H, W, 0, 0) // 8:][:4 * B].view(B, 4)
    assert float(((rec[:, 1] - den).abs() / den).max()) <= 1e-12 and float(((rec[:, 2] - want_v).abs() / want_v).max()) <= 1e-12
    assert float(((rec[:, 3] - scale / (den + V.EPS)).abs() * den).max()) <= 1e-12 * scale


# ------------------------------------------------------------------ 3. flat images
def test_flat_reference_gives_exactly_one_and_leaves_the_destination_bits():
    """y flat under every window: VIF = 1 exactly and the gradient is exactly 0 -- a prefilled gx_add keeps its values; image 1 of the
    same call is a live pair and is added to."""
    _lib, lib = _lib_()
    shape = (2, 3, 48, 61)
    B, Cn, H, W = shape
    x, y = V.mixed_pair(shape, seed=31)
    y[0] = 0.4
    x[0] = 0.2
    scale = 0.25
    want_loss, want, want_v, _ = V.value_and_grad(x, y, 1.0, False, scale)
    assert float(want_v[0]) == 1.0 and int(torch.count_nonzero(want[0])) == 0 and float(want[1].abs().max()) > 0
    g = torch.Generator().manual_seed(5)
    prefill = torch.randn(shape, generator=g) * float(want.abs().max())
    gx, loss = prefill.cuda(), torch.full((1,), 1.5, device="cuda")
    per = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    xd, yd, scratch = x.cuda(), y.cuda(), _scratch(lib, B, Cn, H, W, True)
    _lib.check(lib.m2t_vif_loss_tensor(_lib.ptr(xd), _lib.ptr(yd), B, Cn, H, W, Cn * H * W, W, 1.0, N0, 0, scale, _lib.ptr(gx),
                                       _lib.ptr(loss), _lib.ptr(per), 1, _lib.ptr(scratch), _lib.stream_ptr()), "m2t_vif_loss_tensor")
    torch.cuda.synchronize()
    got = gx.cpu()
    assert torch.equal(got[0], prefill[0])
    assert float(per.cpu()[0]) == 1.0
    nbad, worst = _gate(got.double(), want, prefill=prefill.double())
    assert nbad == 0, (nbad, worst)
    assert abs(float(loss) - 1.5 - float(want_loss)) <= 2.4e-7 * (1.5 + abs(float(want_loss)))
    # a contrast-enhanced x: VIF above 1, the value negative, not clipped
    xe = (1.5 * y[1:]).contiguous().cuda()
    out = torch.zeros(1, device="cuda")
    _lib.check(lib.m2t_vif_loss_tensor(_lib.ptr(xe), _lib.ptr(yd[1:].contiguous()), 1, Cn, H, W, Cn * H * W, W, 1.0, N0, 0, 1.0, None,
                                       _lib.ptr(out), _lib.ptr(per), 0, _lib.ptr(scratch), _lib.stream_ptr()), "m2t_vif_loss_tensor")
    torch.cuda.synchronize()
    assert float(per.cpu()[0]) > 1.0 and float(out) < 0.0


# ------------------------------------------------------------------ 4. the plan entry
def _vif(lib, plan, hr, out, weight=LAM, divisor=None, accumulate=0, scratch=None):
    from m2trans_amd import _lib
    if scratch is None:
        scratch = _scratch(lib, hr.shape[0], 3, hr.shape[-2], hr.shape[-1])
    rc = lib.m2t_vif_loss(plan.handle, _lib.ptr(hr), weight, float(hr.shape[0] if divisor is None else divisor), 1.0, N0, _lib.ptr(out),
                          accumulate, _lib.ptr(scratch), _lib.ptr(plan.workspace), _lib.stream_ptr())
    torch.cuda.synchronize()             # (the scratch of this helper dies with the call)
    return rc


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("scale", [2, 3, 4], ids=["x2-80x112", "x3-120x168", "x4-160x224"])
def test_plan_entry_adds_the_seed_against_fp64(dtype, scale):
    """m2t_pixel_loss(weight 0) then m2t_vif_loss at (1, 40, 56), the smallest reflect-padded shape of the loss tests: ws:gpre against
    the restatement on the read-back bits of ws:srpre; then with the L1 weight 1 the sum of both references."""
    _lib, lib = _lib_()
    B, H, W = 1, 40, 56
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
    tag = f"{dtype} x{scale}"
    inner = pre[..., :Hs, :Ws].cpu()
    assert float(((inner < 0) | (inner > 1)).double().mean()) >= 0.05 and float(((inner >= 0) & (inner <= 1)).double().mean()) >= 0.25, tag
    want_loss, want = V.loss_and_seed(pre.cpu(), hr.cpu(), weight=LAM)
    l1, out = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    # the term alone
    gpre.fill_(float("nan"))
    assert _pixel(lib, plan, hr, l1, weight=0.0) == 0 and _vif(lib, plan, hr, out) == 0
    got = gpre.view(pre.shape).double().cpu()
    assert bool(torch.isfinite(got).all()), tag
    assert int(torch.count_nonzero(got[pad])) == 0, f"{tag}: seed in the padding"
    assert int(torch.count_nonzero(got[clamped])) == 0, f"{tag}: seed where the clamp is active"
    assert int(torch.count_nonzero(want)) > 0.2 * hr.numel()
    nbad, worst = _gate(got[..., :Hs, :Ws], want[..., :Hs, :Ws])
    print(f"{tag}: VIF seed, largest |got - ref| / bound {worst:.3f}; value {float(out):.9e} against {float(want_loss):.9e}")
    assert nbad == 0, f"{tag}: {nbad} seed elements beyond the gate, worst ratio {worst:.3f}"
    assert abs(float(out) - float(want_loss)) <= 1.2e-7 * abs(float(want_loss)), (tag, float(out), float(want_loss))
    # behind the L1 seed
    gpre.fill_(float("nan"))
    assert _pixel(lib, plan, hr, l1, weight=1.0) == 0 and _vif(lib, plan, hr, out) == 0
    got = gpre.view(pre.shape).double().cpu()
    inner = pre[..., :Hs, :Ws].double().cpu()
    d = inner.clamp(0.0, 1.0) - hr.double().cpu()
    seed_l1 = RP.derivative("l1", d) * RP.clamp_mask(inner) * float(torch.tensor(1.0 / hr.numel(), dtype=torch.float32))
    nbad, worst = _gate(got[..., :Hs, :Ws], want[..., :Hs, :Ws], prefill=seed_l1)
    assert nbad == 0, f"{tag}: {nbad} elements of L1 + VIF beyond the gate, worst ratio {worst:.3f}"
    assert int(torch.count_nonzero(got[pad])) == 0 and int(torch.count_nonzero(got[clamped])) == 0, tag


def test_plan_entry_state_and_argument_errors():
    """State rules of m2t_ssim_loss; an SR side < 41 is refused before any launch."""
    _lib, lib = _lib_()
    model = _model(2, "fp32", NB)
    x, hr = _pair(2, "fp32", 1, 40, 56)
    plan = model._plan_for(x)
    out = torch.zeros(1, device="cuda")
    assert _vif(lib, plan, hr, out) == STATE                         # before a forward
    _forward(lib, model, plan, x)
    assert _vif(lib, plan, hr, out) == STATE                         # before any seed
    assert _pixel(lib, plan, hr, out, deferred=True) == 0
    assert _vif(lib, plan, hr, out) == STATE                         # a deferred request leaves no materialised seed
    assert b"materialised" in lib.m2t_last_error_string()
    assert _pixel(lib, plan, hr, out) == 0
    assert _vif(lib, plan, hr, out) == 0
    scratch = _scratch(lib, 1, 3, 80, 112)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    for bad in (dict(hr=None), dict(out=None), dict(scratch=None), dict(ws=None), dict(R=0.0), dict(div=0.0), dict(div=float("nan")),
                dict(n=0.0), dict(n=float("inf"))):
        a = dict(hr=_lib.ptr(hr), out=_lib.ptr(out), scratch=_lib.ptr(scratch), ws=ws, R=1.0, div=1.0, n=N0)
        a.update(bad)
        assert lib.m2t_vif_loss(plan.handle, a["hr"], LAM, a["div"], a["R"], a["n"], a["out"], 0, a["scratch"], a["ws"], st) == ARG, bad
    torch.cuda.synchronize()
    # 20 x 56 at x2: an SR image of 40 x 112
    xs, hs = _images(1, 20, 56, 2)
    small = model._plan_for(xs)
    _forward(lib, model, small, xs)
    assert _pixel(lib, small, hs, out) == 0
    seed = small.ws_tensor("gpre", dtype=torch.float32).clone()
    assert lib.m2t_vif_loss(small.handle, _lib.ptr(hs), LAM, 1.0, 1.0, N0, _lib.ptr(out), 0, _lib.ptr(scratch), _lib.ptr(small.workspace), st) == ARG
    assert b"at least 41" in lib.m2t_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(small.ws_tensor("gpre", dtype=torch.float32), seed)
    assert lib.m2t_vif_loss_scratch_bytes(1, 3, 40, 112) == 0


# ------------------------------------------------------------------ 5. TrainStep against the sequence by hand and against autograd
def _by_hand(model, plan, x, hr, lam=LAM, pix_div=None, vif_div=None):
    """(l1 [1], vif [1], gradients): m2t_forward -> m2t_pixel_loss (l1) -> m2t_vif_loss -> m2t_backward into fresh buffers."""
    _lib, lib = _lib_()
    l1, vf = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    grads = torch.full_like(model.flat_params, float("nan"))
    _forward(lib, model, plan, x)
    assert _pixel(lib, plan, hr, l1, divisor=pix_div) == 0
    assert _vif(lib, plan, hr, vf, weight=lam, divisor=vif_div) == 0
    _backward(lib, model, plan, x, grads)
    torch.cuda.synchronize()
    return l1, vf, grads


@pytest.mark.parametrize("dtype,scale,tol", [("bf16", 4, 1e-2), ("fp32", 2, 1e-5)])
def test_train_step_is_the_sequence_by_hand_and_matches_the_autograd_route(dtype, scale, tol):
    """Two steps with different batches at (2, 40, 56): loss, gradients, parameters and moments bit-identical to m2t_forward ->
    m2t_pixel_loss -> m2t_vif_loss -> m2t_backward -> m2t_adam_step on a twin.  The first step's gradients are also compared with the
    route a user had to take: sr = model(x), torch's L1 plus losses.vif_loss(sr, hr), backward() -- rel-L2 1e-5 in fp32, 1e-2 in bf16,
    the gates of the SSIM and MS-SSIM terms' tests of the same name."""
    from m2trans_amd.losses import vif_loss
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    B, H, W = 2, 40, 56
    m_a, m_b = _model(scale, dtype, NB), _model(scale, dtype, NB)
    ts = TrainStep(m_a, lr=1e-4, world_size=1, lambda_vif=LAM)
    exp_avg, exp_avg_sq = torch.zeros_like(m_b.flat_params), torch.zeros_like(m_b.flat_params)
    first_grads = None
    for step in range(2):
        x, hr = _pair(scale, dtype, B, H, W, step)
        loss = ts.step(x, hr)
        torch.cuda.synchronize()
        plan = m_b._plan_for(x)
        l1, vf, grads = _by_hand(m_b, plan, x, hr)
        if step == 0:
            first_grads = grads.clone()
        n = grads.numel()
        _lib.check(lib.m2t_adam_step(_lib.ptr(m_b.flat_params), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), n, 1e-4, 0.9,
                                     0.999, 1e-8, step + 1, 1.0, _lib.stream_ptr()), "m2t_adam_step")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(grads).all()) and 0 < float(vf) < LAM and float(l1) > 0
        assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.vif_loss, vf) and torch.equal(loss, l1 + vf), (step, float(loss))
        assert ts.loss is loss
        assert list(ts._vif_scratch) == [(B, H * scale, W * scale)]                  # cached per shape
        assert_flat_equal(m_a, ts.grads, grads, f"gradients, step {step}")
        assert_flat_equal(m_a, m_a.flat_params.detach(), m_b.flat_params.detach(), f"parameters, step {step}")
        assert_flat_equal(m_a, ts.exp_avg, exp_avg, f"exp_avg, step {step}")
        assert_flat_equal(m_a, ts.exp_avg_sq, exp_avg_sq, f"exp_avg_sq, step {step}")
    # the autograd route, on the weights of step 0
    model = _model(scale, dtype, NB)
    x, hr = _pair(scale, dtype, B, H, W, 0)
    sr = model(x)
    want_loss = torch.nn.L1Loss()(sr, hr) + LAM * vif_loss(sr, hr)
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
def test_lambda_vif_zero_is_the_default_step_bit_for_bit():
    from m2trans_amd.train_step import TrainStep
    scale, dtype, B, H, W = 4, "bf16", 2, 40, 56
    res = []
    for kw in ({}, {"lambda_vif": 0.0}):
        model = _model(scale, dtype, NB)
        ts = TrainStep(model, lr=1e-4, world_size=1, **kw)
        assert ts.vif_loss is None and ts._vif_scratch == {}
        out = []
        for step in range(2):
            x, hr = _pair(scale, dtype, B, H, W, step)
            loss = ts.step(x, hr)
            torch.cuda.synchronize()
            assert ts.vif_loss is None and loss is ts.l1_loss and ts._vif_scratch == {}
            out.append((loss.clone(), ts.grads.clone(), model.flat_params.detach().clone()))
        res.append((model, out))
    (model, a), (_, b) = res
    for step in range(2):
        assert torch.equal(a[step][0], b[step][0])
        assert_flat_equal(model, a[step][1], b[step][1], f"gradients, step {step}")
        assert_flat_equal(model, a[step][2], b[step][2], f"parameters, step {step}")
    # with the term on, an SR image of 40 x 112 is refused by the step itself, on the host
    from m2trans_amd._lib import M2TError
    with pytest.raises(M2TError, match="at least 41"):
        TrainStep(_model(2, dtype, NB), world_size=1, lambda_vif=LAM).forward_backward(*_images(1, 20, 56, 2))


# ------------------------------------------------------------------ 7. accumulation
def test_accumulated_vif_equals_the_micro_batch_gradients_summed_in_call_order():
    """accum_steps = 2 at micro-batch (1, 40, 56), bf16 x4: the accumulated buffer is the fp32 sum, in call order, of the two
    micro-batch gradients taken by hand with the cycle's divisors (the global number of images: 2); ts.vif_loss is the sum of the two."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    x, hr = _pair(4, "bf16", 2, 40, 56)
    m_a, m_b = _model(4, "bf16", NB), _model(4, "bf16", NB)
    ts = TrainStep(m_a, world_size=1, accum_steps=2, lambda_vif=LAM)
    ts.forward_backward(x[0:1], hr[0:1])
    with pytest.raises(M2TError):
        ts.optimizer_step()                                          # in mid-cycle
    with pytest.raises(M2TError):
        ts.set_lambda_vif(0.0)
    loss = ts.forward_backward(x[1:2], hr[1:2])
    torch.cuda.synchronize()
    parts = []
    for i in range(2):
        cx, chr_ = x[i:i + 1].contiguous(), hr[i:i + 1].contiguous()
        parts.append(_by_hand(m_b, m_b._plan_for(cx), cx, chr_, pix_div=hr.numel(), vif_div=2))
    assert float(parts[1][2].abs().max()) > 0 and float(parts[1][1]) > 0
    assert torch.equal(ts.vif_loss, parts[0][1] + parts[1][1]), (float(ts.vif_loss), float(parts[0][1] + parts[1][1]))
    assert torch.equal(ts.l1_loss, parts[0][0] + parts[1][0])
    assert torch.equal(loss, ts.l1_loss + ts.vif_loss)
    assert_flat_equal(m_a, ts.grads, parts[0][2] + parts[1][2], "accumulated L1 + VIF")
    ts.optimizer_step()
    assert ts.micro_count == 0


# ------------------------------------------------------------------ 8. the four optional terms together
def test_ssim_msssim_fft_and_vif_terms_add_their_seeds():
    """TrainStep(lambda_ssim, lambda_msssim, lambda_fft, lambda_vif) issues pixel -> SSIM -> MS-SSIM -> FFT -> VIF -> backward:
    bit-identical to that sequence by hand; and the seed after the five contributions against the one without VIF plus VIF alone: one
    fp32 add within half an ulp of its sum -> 6e-8 |sum| per element.  48 x 48 at x4: 192 x 192 suits the transform and the five levels."""
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    scale, dtype, B, H, W = 4, "bf16", 1, 48, 48
    x, hr = _pair(scale, dtype, B, H, W)
    Hs = Ws = 192
    lam_s, lam_m, lam_f = 0.1, 0.16, 0.05
    m_a, m_b = _model(scale, dtype, NB), _model(scale, dtype, NB)
    ts = TrainStep(m_a, world_size=1, lambda_ssim=lam_s, lambda_msssim=lam_m, lambda_fft=lam_f, lambda_vif=LAM)
    loss = ts.forward_backward(x, hr)
    torch.cuda.synchronize()
    plan = m_b._plan_for(x)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    l1, ss, ms, ff, vf = (torch.full((1,), float("nan"), device="cuda") for _ in range(5))
    s_ssim = torch.empty(lib.m2t_ssim_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    s_ms = torch.empty(lib.m2t_msssim_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    s_fft = torch.empty(lib.m2t_fft_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    _forward(lib, m_b, plan, x)

    def seed(pixel_weight, others, with_vif):
        assert _pixel(lib, plan, hr, l1, weight=pixel_weight) == 0
        if others:
            _lib.check(lib.m2t_ssim_loss(plan.handle, _lib.ptr(hr), lam_s, float(B * 3 * (Hs - 10) * (Ws - 10)), 1.0, _lib.ptr(ss), 0,
                                         _lib.ptr(s_ssim), ws, st), "m2t_ssim_loss")
            _lib.check(lib.m2t_msssim_loss(plan.handle, _lib.ptr(hr), lam_m, float(B * 3), 1.0, _lib.ptr(ms), 0, _lib.ptr(s_ms), ws, st),
                       "m2t_msssim_loss")
            _lib.check(lib.m2t_fft_loss(plan.handle, _lib.ptr(hr), lam_f, float(B * 3 * Hs * (Ws // 2 + 1) * 2), 1.0, 0, _lib.ptr(ff), 0,
                                        _lib.ptr(s_fft), ws, st), "m2t_fft_loss")
        if with_vif:
            assert _vif(lib, plan, hr, vf) == 0
        torch.cuda.synchronize()
        return gpre.clone()

    before, alone = seed(1.0, True, False).double().cpu(), seed(0.0, False, True).double().cpu()
    assert bool(torch.isfinite(alone).all()) and float(alone.abs().max()) > 0
    full = seed(1.0, True, True).double().cpu()
    excess = (full - (before + alone)).abs() - HALF_ULP * (before + alone).abs()
    assert float(excess.max()) <= 0.0, float(excess.max())
    g_b = torch.full_like(m_b.flat_params, float("nan"))
    _backward(lib, m_b, plan, x, g_b)
    torch.cuda.synchronize()
    assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.ssim_loss, ss) and torch.equal(ts.msssim_loss, ms) and torch.equal(ts.fft_loss, ff)
    assert torch.equal(ts.vif_loss, vf)
    assert torch.equal(loss, ts.l1_loss + ts.ssim_loss + ts.msssim_loss + ts.fft_loss + ts.vif_loss)
    assert_flat_equal(m_a, ts.grads, g_b, "pixel + SSIM + MS-SSIM + FFT + VIF")


# ------------------------------------------------------------------ 9. the autograd Function, the metric and evaluate
def test_vif_loss_function_metric_and_evaluate():
    from m2trans_amd.losses import VIFLoss, vif_loss
    from m2trans_amd.metrics import evaluate, vif_device
    shape = (2, 3, 48, 61)
    x, y = V.mixed_pair(shape, seed=21)
    want_loss, want, want_v, shares = V.value_and_grad(x, y, 1.0, False, 1.0 / shape[0])
    assert min(shares[0].values()) > 0
    leaf = x.cuda().requires_grad_(True)
    got = vif_loss(leaf, y.cuda())
    (got * 3.0).backward()                                          # (an upstream factor reaches the gradient)
    torch.cuda.synchronize()
    assert got.shape == () and abs(float(got.detach()) - float(want_loss)) <= 1.2e-7 * abs(float(want_loss))
    nbad, worst = _gate(leaf.grad.double().cpu() / 3.0, want)
    print(f"vif_loss Function: largest |got - ref| / bound {worst:.3f}")
    # (the division by 3 undoes an fp32 product: one more rounding on each side of it, 1.2e-7 |ref| -- inside the 1e-6 |ref| term)
    assert nbad == 0, (nbad, worst)
    assert float(VIFLoss()(x.cuda(), y.cuda())) == float(got)
    _, _, v7, _ = V.value_and_grad(x, y, 1.0, False, 1.0, 0.7)
    assert abs(float(VIFLoss(sigma_n_sq=0.7)(x.cuda(), y.cuda())) - float((1.0 - v7).mean())) <= 1.2e-7 * abs(float((1.0 - v7).mean()))
    m = vif_device(x.cuda(), y.cuda())
    assert m.dtype == torch.float64 and tuple(m.shape) == (2,)
    assert float(((m.cpu() - want_v).abs() / want_v).max()) <= 1e-12
    m255 = vif_device(x.cuda() * 255.0, y.cuda() * 255.0, data_range=255.0)
    assert float(((m255.cpu() - want_v).abs() / want_v).max()) <= 1e-6           # (x * 255 rounds in fp32)
    grey = vif_device(x[:, :1].contiguous().cuda(), y[:, :1].contiguous().cuda())
    assert float(((grey.cpu() - V.value_and_grad(x[:, :1], y[:, :1])[2]).abs()).max()) <= 1e-12
    # evaluate(with_vif=True): the existing outputs, then the average VIF rounded like FSIM / GMSD
    model = _model(4, "fp32", NB)
    pairs = []
    for step in range(2):
        lr, hr = _pair(4, "fp32", 1, 40, 56, step)
        pairs.append((lr, hr))
    base = evaluate(model, pairs, 4, 1.0)
    with_v = evaluate(model, pairs, 4, 1.0, with_vif=True)
    assert len(base) == 2 and len(with_v) == 3 and with_v[:2] == base
    with torch.no_grad():
        per = torch.cat([vif_device(model(lr), hr, 1.0) for lr, hr in pairs]).cpu()
        ref = torch.cat([V.value_and_grad(model(lr).cpu(), hr.cpu())[2] for lr, hr in pairs])
    assert with_v[2] == round(float(per.sum()) / 2 + 5e-5, 4) and 0.0 < with_v[2] < 1.0
    assert float(((per - ref).abs() / ref).max()) <= 1e-12
    every = evaluate(model, pairs, 4, 1.0, with_gmsd=True, with_fsim=True, with_vif=True)
    assert len(every) == 5 and every[:2] == base and every[4] == with_v[2]
