"""-m gpu: the GMSD loss term (k_gmsd_loss.hip; m2t_gmsd_loss_tensor, m2t_gmsd_loss, losses.gmsd_loss, TrainStep(lambda_gmsd=...))
against the fp64 restatement tests/gmsd_loss_ref.py: the plan-free entry per element, the identical pair, the plan entry on the
forward's own pre-clamp output, TrainStep against the sequence composed by hand, the default step, accumulation, all terms together and
the autograd Function.

The gate of a gradient element is the one of tests/test_gpu_vif_loss.py for the fp64-inside kernels, |got - want| <= 1e-6 |ref| +
1e-7 max_b |ref| + 2^-24 |want| (want = prefill + ref): everything between the fp32 inputs and the single fp32 rounding is fp64, so
what remains is the order of the fp64 sums and one rounding, plus -- where the destination held something -- half an ulp of the sum.
EVERY element is gated.  The value is gated at 1.2e-7 relative (one fp32 rounding), GMSD_b at 1e-12 relative (the restatement asserts
GMSD_b >= 1e-3 for these inputs, so that this is about the kernel and not about conditioning), and at 2e-6 absolute against the fp32
metric metrics.gmsd_device (RGB shapes; the metric takes no other).

Inputs: the "mixed" family of tests/gmsd_loss_ref.py -- a sector exactly 0 in both images, a patch flat in x only, one flat in y only,
about 5 % of x outside [0, R], noise elsewhere.  The tile is 32 x 32 pooled cells: 33 x 70 and 64 x 130 cross a tile edge in width (at
pooled column 32, with at least two cells on both sides), 70 x 33 in height."""
import pytest
import torch

from tests import gmsd_loss_ref as G
from tests import pixel_loss_ref as RP
from tests.gpu_util import assert_flat_equal
from tests.test_gpu_msssim_loss import _hr_for, _model, _pair, _pixel, _srpre
from tests.test_gpu_pixel_loss import _backward, _forward, _images

pytestmark = pytest.mark.gpu

ARG, STATE = -2, -3
LAM = 0.1
NB = 1
HALF_ULP = 2.0 ** -24


def _lib_():
    from m2trans_amd import _lib
    return _lib, _lib.load()


def _scratch(lib, B, Cn, H, W, poison=False):
    n = lib.m2t_gmsd_loss_scratch_bytes(B, Cn, H, W)
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
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return int((err > bound).sum()), float(ratio.max())


# ------------------------------------------------------------------ 1. the plan-free entry against fp64
# (shape, (rows, row stride) of the buffer that holds x or None = contiguous)
CASES = [((1, 1, 2, 2), None),                          # a 1 x 1 map: value 0, the destination's bits untouched
         ((2, 3, 5, 6), None),                          # odd height, a 3 x 3 map: every entry on the zero-padded border
         ((2, 3, 33, 70), (36, 80)),                    # in a NaN-filled buffer, row stride 80, 36 rows; odd height; two tiles wide
         ((1, 3, 70, 33), None),                        # odd width (the scalar path: rows are not 16-byte aligned); two tiles high
         ((1, 1, 64, 130), None)]                       # one channel, three tiles wide (rows aligned in y only)
CASE_IDS = ["2x2", "5x6", "33x70-strided", "70x33", "grey-64x130"]
_REF = {}


def _case(idx, clamp, Rr):
    """Inputs and the reference of one case, computed once and shared (never modified)."""
    key = (idx, clamp, Rr)
    if key not in _REF:
        shape = CASES[idx][0]
        x, y = G.mixed_pair(shape, seed=10 + idx, R=Rr)
        scale = 0.37 / shape[0]
        one_cell = shape[-2:] == (2, 2)
        loss, grad, gm, shares = G.value_and_grad(x, y, Rr, bool(clamp), scale, min_gmsd=None if one_cell else 1e-3)
        assert bool(torch.isfinite(grad).all()), shape
        if one_cell:
            assert float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0
        else:
            assert float(grad.abs().max()) > 0 and int(((x < 0) | (x > Rr)).sum()) > 0
        if min(shape[-2:]) >= 33:
            assert min(shares.values()) > 0 and int(G.sector(shape).sum()) > 0, (shape, shares)
        _REF[key] = (x, y, scale, loss, grad, gm, shares)
    return _REF[key]


RUNS = [(i, c, r) for i in range(len(CASES)) for c in (0, 1) for r in (1.0, 255.0)]


@pytest.mark.parametrize("idx,clamp,Rr", RUNS, ids=[f"{CASE_IDS[i]}-clamp{c}-R{r:g}" for i, c, r in RUNS])
def test_plan_free_entry_against_fp64(idx, clamp, Rr):
    from m2trans_amd.metrics import gmsd_device
    _lib, lib = _lib_()
    shape, layout = CASES[idx]
    B, Cn, H, W = shape
    x, y, scale, want_loss, want, want_g, shares = _case(idx, clamp, Rr)
    rows, rs = layout or (H, W)
    nan = float("nan")
    xbuf = torch.full((B, Cn, rows, rs), nan)                       # what lies outside [H, W] must never be read ...
    xbuf[..., :H, :W] = x
    xbuf, yd = xbuf.cuda(), y.cuda()
    inside = torch.zeros((B, Cn, rows, rs), dtype=torch.bool)
    inside[..., :H, :W] = True
    nan_bits = torch.full((B, Cn, rows, rs), nan).view(torch.int32)
    g = torch.Generator().manual_seed(7)
    noise = (torch.randn((B, Cn, H, W), generator=g) * max(float(want.abs().max()), 1e-3)).float()

    def run(prefill, loss_prefill, accumulate, scratch, with_grad=True):
        gbuf = torch.full((B, Cn, rows, rs), nan)                   # ... nor written
        gbuf[..., :H, :W] = prefill
        gbuf = gbuf.cuda()
        loss = torch.full((1,), loss_prefill, device="cuda")
        per = torch.full((B,), nan, dtype=torch.float64, device="cuda")
        rc = lib.m2t_gmsd_loss_tensor(_lib.ptr(xbuf), _lib.ptr(yd), B, Cn, H, W, Cn * rows * rs, rs, Rr, clamp, scale,
                                      _lib.ptr(gbuf) if with_grad else None, _lib.ptr(loss), _lib.ptr(per), accumulate,
                                      _lib.ptr(scratch), _lib.stream_ptr())
        _lib.check(rc, "m2t_gmsd_loss_tensor")
        torch.cuda.synchronize()
        return gbuf.cpu(), loss.cpu(), per.cpu()

    tag = f"{shape} clamp {clamp} R {Rr:g}"
    g0, l0, p0 = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W))
    got = g0[..., :H, :W].double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(l0).all()), tag
    nbad, worst = _gate(got, want)
    print(f"{tag}: gradient, largest |got - ref| / bound {worst:.3f} (max |ref| {float(want.abs().max()):.3e}); "
          f"value {float(l0):.9e} against {float(want_loss):.9e}; GMSD {want_g.tolist()}; shares {shares}")
    assert nbad == 0, f"{tag}: {nbad} elements beyond the gate, worst ratio {worst:.3f}"
    if clamp:
        assert int(torch.count_nonzero(got[(x < 0) | (x > Rr)])) == 0, f"{tag}: gradient where the clamp is active"
    assert int(torch.count_nonzero(got[G.sector(shape)])) == 0, f"{tag}: gradient on the dead sector"
    # outside [H, W]: bit-unchanged
    assert torch.equal(g0.view(torch.int32)[~inside], nan_bits[~inside]), tag
    # value (within fp32 rounding) and per-image GMSD
    assert abs(float(l0) - float(want_loss)) <= 1.2e-7 * abs(float(want_loss)), (tag, float(l0), float(want_loss))
    if float(want_g.max()) == 0.0:
        assert float(p0.abs().max()) == 0.0 and float(l0) == 0.0, tag
    else:
        perr = float(((p0 - want_g).abs() / want_g).max())
        print(f"{tag}: per_image_out, largest relative error {perr:.3e}")
        assert perr <= 1e-12, (tag, perr)
    if Cn == 3:
        xe = x.clamp(0.0, Rr) if clamp else x
        metric = gmsd_device(xe.cuda(), yd, Rr).cpu()
        merr = float((p0 - metric).abs().max())
        print(f"{tag}: per_image_out against the fp32 metric, largest absolute difference {merr:.3e}")
        assert merr <= 2e-6, (tag, merr)
    # two runs, and a run on poisoned scratch: bit-identical
    for poison in (False, True):
        g1, l1, p1 = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W, poison))
        assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)) and torch.equal(l1, l0) and torch.equal(p1, p0), (tag, poison)
    # value only (gx_add = NULL): the same value, the same per-image numbers
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
    if float(want_g.max()) == 0.0:                                  # the 1 x 1 map: the destination's bits untouched
        assert torch.equal(g3.view(torch.int32), nan_bits) and torch.equal(g2[..., :H, :W].view(torch.int32), noise.view(torch.int32)), tag


@pytest.mark.parametrize("clamp", [0, 1])
def test_identical_pair_leaves_the_destination_bits_and_gives_zero(clamp):
    """Image 0 of the call is identical in x and y: GMSD_0 = 0 exactly and its NaN-prefilled destination keeps every bit; image 1 of
    the same call is a live pair and is added to."""
    _lib, lib = _lib_()
    shape = (2, 3, 33, 70)
    B, Cn, H, W = shape
    x, y = G.mixed_pair(shape, seed=31)
    x[0] = y[0]
    scale = 0.25
    want_loss, want, want_g, _ = G.value_and_grad(x, y, 1.0, bool(clamp), scale)
    assert float(want_g[0]) == 0.0 and float(want_g[1]) >= 1e-3 and int(torch.count_nonzero(want[0])) == 0
    prefill = torch.zeros(shape)
    prefill[0] = float("nan")
    gx, loss = prefill.cuda(), torch.full((1,), 1.5, device="cuda")
    per = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    xd, yd, scratch = x.cuda(), y.cuda(), _scratch(lib, B, Cn, H, W, True)
    _lib.check(lib.m2t_gmsd_loss_tensor(_lib.ptr(xd), _lib.ptr(yd), B, Cn, H, W, Cn * H * W, W, 1.0, clamp, scale, _lib.ptr(gx),
                                        _lib.ptr(loss), _lib.ptr(per), 1, _lib.ptr(scratch), _lib.stream_ptr()), "m2t_gmsd_loss_tensor")
    torch.cuda.synchronize()
    got = gx.cpu()
    assert torch.equal(got[0].view(torch.int32), prefill[0].view(torch.int32))
    assert float(per.cpu()[0]) == 0.0 and abs(float(per.cpu()[1]) - float(want_g[1])) <= 1e-12 * float(want_g[1])
    nbad, worst = _gate(got[1:].double(), want[1:])
    assert nbad == 0, (nbad, worst)
    assert abs(float(loss) - 1.5 - float(want_loss)) <= 2.4e-7 * (1.5 + abs(float(want_loss)))


# ------------------------------------------------------------------ 2. the plan entry
def _gmsd(lib, plan, hr, out, weight=LAM, divisor=None, accumulate=0, scratch=None):
    from m2trans_amd import _lib
    if scratch is None:
        scratch = _scratch(lib, hr.shape[0], 3, hr.shape[-2], hr.shape[-1])
    rc = lib.m2t_gmsd_loss(plan.handle, _lib.ptr(hr), weight, float(hr.shape[0] if divisor is None else divisor), 1.0, _lib.ptr(out),
                           accumulate, _lib.ptr(scratch), _lib.ptr(plan.workspace), _lib.stream_ptr())
    torch.cuda.synchronize()             # (the scratch of this helper dies with the call)
    return rc


def _seed_ref(pre, hr, weight=LAM):
    """The restatement's value and seed on the read-back pre-clamp output (padded size): clamp on, R = 1, scale = weight / B."""
    Hs, Ws = hr.shape[-2:]
    loss, grad, gm, _ = G.value_and_grad(pre[..., :Hs, :Ws].cpu(), hr.cpu(), 1.0, True, weight / hr.shape[0], min_gmsd=1e-3)
    return loss, grad


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("scale,lr", [(2, (20, 28)), (3, (21, 27)), (4, (20, 27))], ids=["x2-40x56", "x3-63x81", "x4-80x108"])
def test_plan_entry_adds_the_seed_against_fp64(dtype, scale, lr):
    """m2t_l1_loss then m2t_gmsd_loss, one block: ws:gpre equals the L1 seed plus the restatement's gradient of the run's own pre-clamp
    output, within the gate; exactly 0 in the padding and where the clamp is active.  x3 gives SR 63 x 81, odd on both sides."""
    _lib, lib = _lib_()
    B, (H, W) = 1, lr
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
    want_loss, want = _seed_ref(pre, hr)
    assert float(want.abs().max()) > 0
    l1, out = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    # the term alone (an L1 seed of weight 0)
    gpre.fill_(float("nan"))
    assert _pixel(lib, plan, hr, l1, weight=0.0) == 0 and _gmsd(lib, plan, hr, out) == 0
    got = gpre.view(pre.shape).double().cpu()
    assert bool(torch.isfinite(got).all()), tag
    assert int(torch.count_nonzero(got[pad])) == 0, f"{tag}: seed in the padding"
    assert int(torch.count_nonzero(got[clamped])) == 0, f"{tag}: seed where the clamp is active"
    nbad, worst = _gate(got[..., :Hs, :Ws], want)
    print(f"{tag}: GMSD seed, largest |got - ref| / bound {worst:.3f}; value {float(out):.9e} against {float(want_loss):.9e}")
    assert nbad == 0, f"{tag}: {nbad} seed elements beyond the gate, worst ratio {worst:.3f}"
    assert abs(float(out) - float(want_loss)) <= 1.2e-7 * abs(float(want_loss)), (tag, float(out), float(want_loss))
    # behind the L1 seed, through m2t_l1_loss
    gpre.fill_(float("nan"))
    _lib.check(lib.m2t_l1_loss(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(l1), _lib.ptr(plan.workspace),
                               _lib.stream_ptr()), "m2t_l1_loss")
    assert _gmsd(lib, plan, hr, out) == 0
    got = gpre.view(pre.shape).double().cpu()
    inner = pre[..., :Hs, :Ws].double().cpu()
    d = inner.clamp(0.0, 1.0) - hr.double().cpu()
    seed_l1 = RP.derivative("l1", d) * RP.clamp_mask(inner) * float(torch.tensor(1.0 / hr.numel(), dtype=torch.float32))
    nbad, worst = _gate(got[..., :Hs, :Ws], want, prefill=seed_l1)
    assert nbad == 0, f"{tag}: {nbad} elements of L1 + GMSD beyond the gate, worst ratio {worst:.3f}"
    assert int(torch.count_nonzero(got[pad])) == 0 and int(torch.count_nonzero(got[clamped])) == 0, tag


def test_plan_entry_state_and_argument_errors():
    """State rules of m2t_ssim_loss; the argument refusals come before any launch."""
    _lib, lib = _lib_()
    model = _model(2, "fp32", NB)
    x, hr = _pair(2, "fp32", 1, 20, 28)
    plan = model._plan_for(x)
    out = torch.zeros(1, device="cuda")
    assert _gmsd(lib, plan, hr, out) == STATE                        # before a forward
    _forward(lib, model, plan, x)
    assert _gmsd(lib, plan, hr, out) == STATE                        # before any seed
    assert _pixel(lib, plan, hr, out, deferred=True) == 0
    assert _gmsd(lib, plan, hr, out) == STATE                        # a deferred request leaves no materialised seed
    assert b"materialised" in lib.m2t_last_error_string()
    assert _pixel(lib, plan, hr, out) == 0
    seed = plan.ws_tensor("gpre", dtype=torch.float32).clone()
    scratch = _scratch(lib, 1, 3, 40, 56)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    for bad in (dict(hr=None), dict(out=None), dict(scratch=None), dict(ws=None), dict(R=0.0), dict(R=float("inf")), dict(div=0.0),
                dict(div=float("nan")), dict(w=float("nan"))):
        a = dict(hr=_lib.ptr(hr), out=_lib.ptr(out), scratch=_lib.ptr(scratch), ws=ws, R=1.0, div=1.0, w=LAM)
        a.update(bad)
        assert lib.m2t_gmsd_loss(plan.handle, a["hr"], a["w"], a["div"], a["R"], a["out"], 0, a["scratch"], a["ws"], st) == ARG, bad
    assert lib.m2t_gmsd_loss(None, _lib.ptr(hr), LAM, 1.0, 1.0, _lib.ptr(out), 0, _lib.ptr(scratch), ws, st) == ARG
    torch.cuda.synchronize()
    assert torch.equal(plan.ws_tensor("gpre", dtype=torch.float32), seed)        # a refused call touches nothing
    assert _gmsd(lib, plan, hr, out) == 0 and float(out) > 0


# ------------------------------------------------------------------ 3. TrainStep against the sequence by hand
def _by_hand(model, plan, x, hr, lam=LAM, pix_div=None, gmsd_div=None):
    """(l1 [1], gmsd [1], gradients): m2t_forward -> m2t_pixel_loss (l1) -> m2t_gmsd_loss -> m2t_backward into fresh buffers."""
    _lib, lib = _lib_()
    l1, gm = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    grads = torch.full_like(model.flat_params, float("nan"))
    _forward(lib, model, plan, x)
    assert _pixel(lib, plan, hr, l1, divisor=pix_div) == 0
    assert _gmsd(lib, plan, hr, gm, weight=lam, divisor=gmsd_div) == 0
    _backward(lib, model, plan, x, grads)
    torch.cuda.synchronize()
    return l1, gm, grads


@pytest.mark.parametrize("dtype,scale", [("bf16", 4), ("fp32", 2)])
def test_train_step_is_the_sequence_by_hand(dtype, scale):
    """Two steps with different batches at (2, 20, 28): loss, gradients, parameters and moments bit-identical to m2t_forward ->
    m2t_pixel_loss -> m2t_gmsd_loss -> m2t_backward -> m2t_adam_step on a twin; the term is live."""
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    B, H, W = 2, 20, 28
    m_a, m_b = _model(scale, dtype, NB), _model(scale, dtype, NB)
    ts = TrainStep(m_a, lr=1e-4, world_size=1, lambda_gmsd=LAM)
    exp_avg, exp_avg_sq = torch.zeros_like(m_b.flat_params), torch.zeros_like(m_b.flat_params)
    first_grads = None
    for step in range(2):
        x, hr = _pair(scale, dtype, B, H, W, step)
        loss = ts.step(x, hr)
        torch.cuda.synchronize()
        plan = m_b._plan_for(x)
        l1, gm, grads = _by_hand(m_b, plan, x, hr)
        if step == 0:
            first_grads = grads.clone()
        n = grads.numel()
        _lib.check(lib.m2t_adam_step(_lib.ptr(m_b.flat_params), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), n, 1e-4, 0.9,
                                     0.999, 1e-8, step + 1, 1.0, _lib.stream_ptr()), "m2t_adam_step")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(grads).all()) and 0 < float(gm) < LAM and float(l1) > 0
        assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.gmsd_loss, gm) and torch.equal(loss, l1 + gm), (step, float(loss))
        assert ts.loss is loss
        assert list(ts._gmsd_scratch) == [(B, H * scale, W * scale)]                 # cached per shape
        assert_flat_equal(m_a, ts.grads, grads, f"gradients, step {step}")
        assert_flat_equal(m_a, m_a.flat_params.detach(), m_b.flat_params.detach(), f"parameters, step {step}")
        assert_flat_equal(m_a, ts.exp_avg, exp_avg, f"exp_avg, step {step}")
        assert_flat_equal(m_a, ts.exp_avg_sq, exp_avg_sq, f"exp_avg_sq, step {step}")
    # the term is live: the L1 step alone gives other gradients
    x, hr = _pair(scale, dtype, B, H, W, 0)
    ts0 = TrainStep(_model(scale, dtype, NB), world_size=1)
    ts0.forward_backward(x, hr)
    torch.cuda.synchronize()
    assert not torch.equal(ts0.grads, first_grads)


def test_lambda_gmsd_zero_is_the_default_step_bit_for_bit():
    from m2trans_amd.train_step import TrainStep
    scale, dtype, B, H, W = 4, "bf16", 2, 20, 28
    res = []
    for kw in ({}, {"lambda_gmsd": 0.0}):
        model = _model(scale, dtype, NB)
        ts = TrainStep(model, lr=1e-4, world_size=1, **kw)
        assert ts.gmsd_loss is None and ts._gmsd_scratch == {}
        out = []
        for step in range(2):
            x, hr = _pair(scale, dtype, B, H, W, step)
            loss = ts.step(x, hr)
            torch.cuda.synchronize()
            assert ts.gmsd_loss is None and loss is ts.l1_loss and ts._gmsd_scratch == {}
            out.append((loss.clone(), ts.grads.clone(), model.flat_params.detach().clone()))
        res.append((model, out))
    (model, a), (_, b) = res
    for step in range(2):
        assert torch.equal(a[step][0], b[step][0])
        assert_flat_equal(model, a[step][1], b[step][1], f"gradients, step {step}")
        assert_flat_equal(model, a[step][2], b[step][2], f"parameters, step {step}")


def test_accumulated_gmsd_equals_the_micro_batch_gradients_summed_in_call_order():
    """accum_steps = 2 at micro-batch (1, 20, 28), bf16 x4: the accumulated buffer is the fp32 sum, in call order, of the two
    micro-batch gradients taken by hand with the cycle's divisors (the global number of images: 2); ts.gmsd_loss is the sum of the two."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    x, hr = _pair(4, "bf16", 2, 20, 28)
    m_a, m_b = _model(4, "bf16", NB), _model(4, "bf16", NB)
    ts = TrainStep(m_a, world_size=1, accum_steps=2, lambda_gmsd=LAM)
    ts.forward_backward(x[0:1], hr[0:1])
    with pytest.raises(M2TError):
        ts.optimizer_step()                                          # in mid-cycle
    with pytest.raises(M2TError):
        ts.set_lambda_gmsd(0.0)
    loss = ts.forward_backward(x[1:2], hr[1:2])
    torch.cuda.synchronize()
    parts = []
    for i in range(2):
        cx, chr_ = x[i:i + 1].contiguous(), hr[i:i + 1].contiguous()
        parts.append(_by_hand(m_b, m_b._plan_for(cx), cx, chr_, pix_div=hr.numel(), gmsd_div=2))
    assert float(parts[1][2].abs().max()) > 0 and float(parts[1][1]) > 0
    assert torch.equal(ts.gmsd_loss, parts[0][1] + parts[1][1]), (float(ts.gmsd_loss), float(parts[0][1] + parts[1][1]))
    assert torch.equal(ts.l1_loss, parts[0][0] + parts[1][0])
    assert torch.equal(loss, ts.l1_loss + ts.gmsd_loss)
    assert_flat_equal(m_a, ts.grads, parts[0][2] + parts[1][2], "accumulated L1 + GMSD")
    ts.optimizer_step()
    assert ts.micro_count == 0


def test_all_terms_together_add_their_seeds():
    """TrainStep(lambda_ssim, lambda_msssim, lambda_fft, lambda_vif, lambda_gmsd) issues pixel -> SSIM -> MS-SSIM -> FFT -> VIF -> GMSD ->
    backward: bit-identical to that sequence by hand; and the seed after the six contributions against the one without GMSD plus GMSD
    alone: one fp32 add within half an ulp of its sum.  48 x 48 at x4: 192 x 192 suits the transform and the five levels."""
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    scale, dtype, B, H, W = 4, "bf16", 1, 48, 48
    x, hr = _pair(scale, dtype, B, H, W)
    Hs = Ws = 192
    lam_s, lam_m, lam_f, lam_v = 0.1, 0.16, 0.05, 0.1
    m_a, m_b = _model(scale, dtype, NB), _model(scale, dtype, NB)
    ts = TrainStep(m_a, world_size=1, lambda_ssim=lam_s, lambda_msssim=lam_m, lambda_fft=lam_f, lambda_vif=lam_v, lambda_gmsd=LAM)
    loss = ts.forward_backward(x, hr)
    torch.cuda.synchronize()
    plan = m_b._plan_for(x)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    l1, ss, ms, ff, vf, gm = (torch.full((1,), float("nan"), device="cuda") for _ in range(6))
    s_ssim = torch.empty(lib.m2t_ssim_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    s_ms = torch.empty(lib.m2t_msssim_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    s_fft = torch.empty(lib.m2t_fft_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    s_vif = torch.empty(lib.m2t_vif_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    _forward(lib, m_b, plan, x)

    def seed(pixel_weight, others, with_gmsd):
        assert _pixel(lib, plan, hr, l1, weight=pixel_weight) == 0
        if others:
            _lib.check(lib.m2t_ssim_loss(plan.handle, _lib.ptr(hr), lam_s, float(B * 3 * (Hs - 10) * (Ws - 10)), 1.0, _lib.ptr(ss), 0,
                                         _lib.ptr(s_ssim), ws, st), "m2t_ssim_loss")
            _lib.check(lib.m2t_msssim_loss(plan.handle, _lib.ptr(hr), lam_m, float(B * 3), 1.0, _lib.ptr(ms), 0, _lib.ptr(s_ms), ws, st),
                       "m2t_msssim_loss")
            _lib.check(lib.m2t_fft_loss(plan.handle, _lib.ptr(hr), lam_f, float(B * 3 * Hs * (Ws // 2 + 1) * 2), 1.0, 0, _lib.ptr(ff), 0,
                                        _lib.ptr(s_fft), ws, st), "m2t_fft_loss")
            _lib.check(lib.m2t_vif_loss(plan.handle, _lib.ptr(hr), lam_v, float(B), 1.0, _lib.VIF_SIGMA_N_SQ, _lib.ptr(vf), 0,
                                        _lib.ptr(s_vif), ws, st), "m2t_vif_loss")
        if with_gmsd:
            assert _gmsd(lib, plan, hr, gm) == 0
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
    assert torch.equal(ts.vif_loss, vf) and torch.equal(ts.gmsd_loss, gm)
    assert torch.equal(loss, ts.l1_loss + ts.ssim_loss + ts.msssim_loss + ts.fft_loss + ts.vif_loss + ts.gmsd_loss)
    assert_flat_equal(m_a, ts.grads, g_b, "pixel + SSIM + MS-SSIM + FFT + VIF + GMSD")


# ------------------------------------------------------------------ 4. the autograd Function
def test_gmsd_loss_function_gives_the_restatements_gradient():
    from m2trans_amd.losses import GMSDLoss, gmsd_loss
    shape = (2, 3, 33, 70)
    x, y = G.mixed_pair(shape, seed=21)
    want_loss, want, want_g, shares = G.value_and_grad(x, y, 1.0, False, 1.0 / shape[0], min_gmsd=1e-3)
    assert min(shares.values()) > 0
    leaf = x.cuda().requires_grad_(True)
    got = gmsd_loss(leaf, y.cuda())
    (got * 3.0).backward()                                          # (an upstream factor reaches the gradient)
    torch.cuda.synchronize()
    assert got.shape == () and abs(float(got.detach()) - float(want_loss)) <= 1.2e-7 * abs(float(want_loss))
    assert bool(torch.isfinite(leaf.grad).all())
    nbad, worst = _gate(leaf.grad.double().cpu() / 3.0, want)
    print(f"gmsd_loss Function: largest |got - ref| / bound {worst:.3f}")
    # (the division by 3 undoes an fp32 product: one more rounding on each side of it, 1.2e-7 |ref| -- inside the 1e-6 |ref| term)
    assert nbad == 0, (nbad, worst)
    assert int(torch.count_nonzero(leaf.grad.cpu()[G.sector(shape)])) == 0
    assert float(GMSDLoss()(x.cuda(), y.cuda())) == float(got.detach())
    w255, _, _, _ = G.value_and_grad(x * 255.0, y * 255.0, 255.0, False, 1.0 / shape[0])
    assert abs(float(GMSDLoss(255.0)(x.cuda() * 255.0, y.cuda() * 255.0)) - float(w255)) <= 1.2e-7 * abs(float(w255))
