"""-m gpu: the wavelet-domain loss term (k_wavelet_loss.hip; m2t_swt2, m2t_wavelet_loss_tensor, m2t_wavelet_loss, losses.swt2 /
wavelet_loss, TrainStep(lambda_wavelet=...)) against the fp64 restatement tests/wavelet_loss_ref.py: the transform alone per
coefficient, the plan-free entry per element, the zero sector and the zero weights, the plan entry on the forward's own pre-clamp
output, TrainStep against the sequence composed by hand, the default step, accumulation, all terms together and the autograd Function.

Gates.  A coefficient of m2t_swt2: |got - ref| <= 2^-24 |ref| + 1e-12 max|d| -- the one fp32 rounding, plus 100 times the 1e-14 max|d|
that 6 L fp64 roundings through six passes of gain sum|f| <= 1.19 can leave.  A gradient element: the gate of tests/test_gpu_vif_loss.py
for the fp64-inside kernels, |got - want| <= 1e-6 |ref| + 1e-7 max_b |ref| + 2^-24 |want| (want = prefill + ref); EVERY element is
gated.  The value at 1.2e-7 relative (one fp32 rounding), the band sums at 1e-12 relative.  For eps = 0 the restatement asserts its
own conditioning (every coefficient of a weighted band is exactly 0 on an all-zero support or has |c| >= 1e-9), so that a sign is
never a matter of rounding.

Inputs: the "mixed" family of tests/wavelet_loss_ref.py -- a sector exactly 0 in both images, about 5 % of x outside [0, R], noise
elsewhere.  The tile is 32 x 32 coefficients: 33 x 70, 70 x 33 and 64 x 130 cross tile edges through the periodic wrap; 56 x 72 (db2,
three levels: a reach of 21) crosses one in each axis with more than the cascade's reach on both sides of it.  The kernels come in two
variants, staging a reach per pass of at most 12 or of up to 28: the shapes the issue lists all take the first, the two 8-tap cases the
second."""
import pytest
import torch

from tests import pixel_loss_ref as RP
from tests import wavelet_loss_ref as Wv
from tests.gpu_util import assert_flat_equal
from tests.test_gpu_msssim_loss import _hr_for, _model, _pair, _pixel, _srpre
from tests.test_gpu_pixel_loss import _backward, _forward, _images

pytestmark = pytest.mark.gpu

ARG, STATE = -2, -3
LAM = 0.1
NB = 1
HALF_ULP = 2.0 ** -24
NAN = float("nan")


def _lib_():
    from m2trans_amd import _lib
    return _lib, _lib.load()


def _args(name, J, weights=None, eps=0.0):
    """The wavelet arguments of the C entries: lo, hi, taps, levels, band_weights, eps."""
    from m2trans_amd.train_step import resolve_wavelet, wavelet_call_args
    lo, hi = Wv.FILTERS[name]
    return wavelet_call_args(resolve_wavelet(name if name in ("haar", "db2") else (lo, hi), J, weights, eps))


def _scratch(lib, B, Cn, H, W, J, taps, poison=False):
    n = lib.m2t_wavelet_loss_scratch_bytes(B, Cn, H, W, J, taps)
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


# (shape, filter, levels, (rows, row stride) of the buffer that holds x or None = contiguous)
CASES = [((1, 1, 2, 2), "haar", 1, None),               # the minimum size
         ((2, 3, 13, 14), "db2", 3, None),              # the minimum side: every level-3 tap wraps
         ((2, 3, 33, 70), "db2", 3, (36, 80)),          # in a NaN-filled buffer of 36 rows, row stride 80
         ((1, 3, 70, 33), "haar", 3, None),             # odd width: the unaligned path
         ((1, 1, 64, 130), "tri", 2, None),             # one channel, the 3-tap pair
         ((1, 3, 56, 72), "db2", 3, None),              # a tile edge in each axis with the cascade's reach (21) on both sides
         ((1, 1, 29, 40), "tap8", 3, None),             # 8 taps at the minimum side: the variant of the tile for a reach above 12
         ((1, 3, 40, 29), "tap8", 2, (40, 32))]         # ... and both variants in one call (a reach of 7, then of 14)
CASE_IDS = ["2x2-haar1", "13x14-db2", "33x70-strided-db2", "70x33-haar", "grey-64x130-tri", "56x72-db2", "grey-29x40-tap8", "40x29-tap8"]
_REF = {}


def _case(idx, clamp, Rr, eps):
    """Inputs and the reference of one case, computed once and shared (never modified)."""
    key = (idx, clamp, Rr, eps)
    if key not in _REF:
        shape, name, J, _ = CASES[idx]
        lo, hi = Wv.FILTERS[name]
        x, y = Wv.mixed_pair(shape, seed=10 + idx, R=Rr)
        B, Cn, H, W = shape
        scale = 0.37 / (B * Cn * H * W)
        loss, grad, sums, smallest = Wv.value_and_grad(x, y, Rr, bool(clamp), scale, lo, hi, J, None, eps)
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0, shape
        if H * W >= 100:
            assert int(((x < 0) | (x > Rr)).sum()) > 0
        _REF[key] = (x, y, scale, loss, grad, sums, smallest)
    return _REF[key]


# ------------------------------------------------------------------ 1. the transform alone
@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_swt2_every_coefficient_against_fp64(idx):
    from m2trans_amd.losses import swt2
    _lib, lib = _lib_()
    shape, name, J, layout = CASES[idx]
    B, Cn, H, W = shape
    lo, hi = Wv.FILTERS[name]
    x, _ = Wv.mixed_pair(shape, seed=40 + idx)
    ref = torch.stack(Wv.swt2(x.double(), lo, hi, J), dim=2)                 # [B,C,3J+1,H,W]
    rows, rs = layout or (H, W)
    xbuf = torch.full((B, Cn, rows, rs), NAN)
    xbuf[..., :H, :W] = x
    xbuf = xbuf.cuda()
    a = _args(name, J)
    outs = []
    for poison in (False, True):
        out = torch.full((B, Cn, 3 * J + 1, H, W), NAN, device="cuda")
        _lib.check(lib.m2t_swt2(_lib.ptr(xbuf), B, Cn, H, W, Cn * rows * rs, rs, a[0], a[1], a[2], a[3], _lib.ptr(out),
                                _lib.ptr(_scratch(lib, B, Cn, H, W, J, a[2], poison)), _lib.stream_ptr()), "m2t_swt2")
        torch.cuda.synchronize()
        outs.append(out.cpu())
    got = outs[0].double()
    assert bool(torch.isfinite(got).all())
    bound = HALF_ULP * ref.abs() + 1e-12 * float(x.abs().max())
    ratio = float(((got - ref).abs() / bound).max())
    print(f"{shape} {name} J={J}: swt2, largest |got - ref| / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))       # bit-reproducible, whatever the scratch held
    if name in ("haar", "db2") and layout is None:              # the Python entry, by name
        py = swt2(x.cuda(), name, J).cpu()
        assert py.shape == (B, Cn, 3 * J + 1, H, W) and torch.equal(py.view(torch.int32), outs[0].view(torch.int32))


# ------------------------------------------------------------------ 2. the plan-free entry against fp64
RUNS = [(i, c, r, e) for i in range(len(CASES)) for c in (0, 1) for r in (1.0, 255.0) for e in (0.0, 1e-3)]


@pytest.mark.parametrize("idx,clamp,Rr,eps", RUNS, ids=[f"{CASE_IDS[i]}-clamp{c}-R{r:g}-eps{e:g}" for i, c, r, e in RUNS])
def test_plan_free_entry_against_fp64(idx, clamp, Rr, eps):
    _lib, lib = _lib_()
    shape, name, J, layout = CASES[idx]
    B, Cn, H, W = shape
    nb = 3 * J + 1
    x, y, scale, want_loss, want, want_s, smallest = _case(idx, clamp, Rr, eps)
    a = _args(name, J, None, eps)
    rows, rs = layout or (H, W)
    xbuf = torch.full((B, Cn, rows, rs), NAN)                       # what lies outside [H, W] must never be read ...
    xbuf[..., :H, :W] = x
    xbuf, yd = xbuf.cuda(), y.cuda()
    inside = torch.zeros((B, Cn, rows, rs), dtype=torch.bool)
    inside[..., :H, :W] = True
    nan_bits = torch.full((B, Cn, rows, rs), NAN).view(torch.int32)
    g = torch.Generator().manual_seed(7)
    noise = (torch.randn((B, Cn, H, W), generator=g) * float(want.abs().max())).float()

    def run(prefill, loss_prefill, accumulate, poison=False, with_grad=True):
        gbuf = torch.full((B, Cn, rows, rs), NAN)                   # ... nor written
        gbuf[..., :H, :W] = prefill
        gbuf = gbuf.cuda()
        loss = torch.full((1,), loss_prefill, device="cuda")
        per = torch.full((nb,), NAN, dtype=torch.float64, device="cuda")
        scratch = _scratch(lib, B, Cn, H, W, J, a[2], poison)
        rc = lib.m2t_wavelet_loss_tensor(_lib.ptr(xbuf), _lib.ptr(yd), B, Cn, H, W, Cn * rows * rs, rs, Rr, clamp, scale, *a,
                                         _lib.ptr(gbuf) if with_grad else None, _lib.ptr(loss), _lib.ptr(per), accumulate,
                                         _lib.ptr(scratch), _lib.stream_ptr())
        _lib.check(rc, "m2t_wavelet_loss_tensor")
        torch.cuda.synchronize()
        return gbuf.cpu(), loss.cpu(), per.cpu()

    tag = f"{shape} {name} J={J} clamp {clamp} R {Rr:g} eps {eps:g}"
    g0, l0, p0 = run(0.0, NAN, 0)
    got = g0[..., :H, :W].double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(l0).all()), tag
    nbad, worst = _gate(got, want)
    print(f"{tag}: gradient, largest |got - ref| / bound {worst:.3f} (max |ref| {float(want.abs().max()):.3e}); "
          f"value {float(l0):.9e} against {want_loss:.9e}; smallest non-zero |c| {smallest:.3g}")
    assert nbad == 0, f"{tag}: {nbad} elements beyond the gate, worst ratio {worst:.3f}"
    # outside [H, W]: bit-unchanged
    assert torch.equal(g0.view(torch.int32)[~inside], nan_bits[~inside]), tag
    # value (within fp32 rounding) and the band sums
    assert abs(float(l0) - want_loss) <= 1.2e-7 * abs(want_loss), (tag, float(l0), want_loss)
    perr = float(((p0 - want_s).abs() - 1e-12 * want_s.abs()).max())
    assert perr <= 0.0 and float(p0[3 * J]) == 0.0, (tag, p0.tolist(), want_s.tolist())       # (LL has weight 0: no sum is formed)
    # two runs, and a run on poisoned scratch: bit-identical
    for poison in (False, True):
        g1, l1, p1 = run(0.0, NAN, 0, poison)
        assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)) and torch.equal(l1, l0) and torch.equal(p1, p0), (tag, poison)
    # value only (gx_add = NULL): the same value, the same band sums
    _, lv, pv = run(NAN, NAN, 0, True, with_grad=False)
    assert torch.equal(lv, l0) and torch.equal(pv, p0), tag
    # a prefilled destination is added to, in the gradient and (accumulate = 1) in the value
    g2, l2, _ = run(noise, 2.5, 1)
    nbad, worst = _gate(g2[..., :H, :W].double(), want, prefill=noise.double())
    assert nbad == 0, f"{tag}: {nbad} elements of the prefilled destination beyond the gate, worst ratio {worst:.3f}"
    assert torch.equal(g2[..., :H, :W], noise + g0[..., :H, :W]), tag          # (the same fp32 add)
    assert torch.equal(l2, torch.tensor([2.5]) + l0), (tag, float(l2), float(l0))
    # elements the clamp holds back keep their bits
    if clamp:
        held = (x < 0) | (x > Rr)
        g3, _, _ = run(NAN, NAN, 0)
        assert torch.equal(g3[..., :H, :W][held].view(torch.int32), nan_bits[..., :H, :W][held]), tag
        assert int(torch.count_nonzero(got[held])) == 0, tag


# ------------------------------------------------------------------ 3. the zero sector and the zero weights
@pytest.mark.parametrize("eps", [0.0, 1e-3])
def test_the_zero_sector_is_not_touched_and_a_zero_weight_is_the_band_left_out(eps):
    """70 x 33, haar, three levels, the sector half the image: no gradient element whose whole reach lies in the sector is changed
    (a destination of -0.0 would become +0.0 under an add of 0); weights with zeros -- two detail bands, the whole of level 2 in a
    second run -- against the restatement that leaves those bands out; LL weighted."""
    _lib, lib = _lib_()
    shape, J = (1, 3, 70, 33), 3
    B, Cn, H, W = shape
    lo, hi = Wv.HAAR
    x, y = Wv.mixed_pair(shape, seed=50, div=2)
    sec = Wv.sector(shape, 2, J, div=2)
    assert int(sec.sum()) > 0
    xd, yd = x.cuda(), y.cuda()
    scale = 1.0 / x.numel()
    for weights, skip in (([1.0, 0.0, 2.0, 0.5, 1.0, 0.0, 1.0, 1.0, 1.0, 0.25], (1, 5)),
                          ([1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 2.0, 1.0, 0.0], (3, 4, 5)),
                          ([1.0, 0.5, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], (3, 4, 5, 6, 7, 8))):
        full = [w if w > 0 else 1.0 for w in weights[:9]] + [weights[9]]
        want_loss, want, want_s, _ = Wv.value_and_grad(x, y, 1.0, True, scale, lo, hi, J, full, eps, skip=skip)
        a = _args("haar", J, weights, eps)
        gx = torch.full(shape, -0.0, device="cuda")
        loss = torch.full((1,), NAN, device="cuda")
        per = torch.full((10,), NAN, dtype=torch.float64, device="cuda")
        _lib.check(lib.m2t_wavelet_loss_tensor(_lib.ptr(xd), _lib.ptr(yd), B, Cn, H, W, Cn * H * W, W, 1.0, 1, scale, *a, _lib.ptr(gx),
                                               _lib.ptr(loss), _lib.ptr(per), 0, _lib.ptr(_scratch(lib, B, Cn, H, W, J, 2, True)),
                                               _lib.stream_ptr()), "m2t_wavelet_loss_tensor")
        torch.cuda.synchronize()
        got = gx.cpu()
        minus_zero = torch.full(shape, -0.0).view(torch.int32)
        assert torch.equal(got.view(torch.int32)[sec], minus_zero[sec]), weights
        nbad, worst = _gate(got.double(), want)
        print(f"weights {weights} eps {eps:g}: largest |got - ref| / bound {worst:.3f}")
        assert nbad == 0, (weights, nbad, worst)
        assert abs(float(loss) - want_loss) <= 1.2e-7 * abs(want_loss)
        p = per.cpu()
        assert float(((p - want_s).abs() - 1e-12 * want_s.abs()).max()) <= 0.0 and all(float(p[b]) == 0.0 for b in skip)


# ------------------------------------------------------------------ 4. the plan entry
WAVE = ("db2", 2)


def _wavelet(lib, plan, hr, out, weight=LAM, divisor=None, accumulate=0, args=None, scratch=None):
    from m2trans_amd import _lib
    a = args or _args(*WAVE)
    if scratch is None:
        scratch = _scratch(lib, hr.shape[0], 3, hr.shape[-2], hr.shape[-1], a[3], a[2])
    rc = lib.m2t_wavelet_loss(plan.handle, _lib.ptr(hr), weight, float(hr.numel() if divisor is None else divisor), 1.0, *a,
                              _lib.ptr(out), accumulate, _lib.ptr(scratch), _lib.ptr(plan.workspace), _lib.stream_ptr())
    torch.cuda.synchronize()             # (the scratch of this helper dies with the call)
    return rc


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_plan_entry_adds_the_seed_against_fp64(dtype):
    """m2t_pixel_loss then m2t_wavelet_loss, one block, x2 at 20 x 28 (SR 40 x 56 in a reflect-padded buffer): ws:gpre equals the L1
    seed plus the restatement's gradient of the run's own pre-clamp output, within the gate; exactly 0 in the padding and where the
    clamp is active."""
    _lib, lib = _lib_()
    scale, B, (H, W) = 2, 1, (20, 28)
    model = _model(scale, dtype, NB)
    x, _ = _images(B, H, W, scale)
    plan = model._plan_for(x)
    _forward(lib, model, plan, x)
    torch.cuda.synchronize()
    pre = _srpre(plan, B, scale).clone()
    Hs, Ws = H * scale, W * scale
    hr = _hr_for(pre, Hs, Ws)
    assert tuple(pre.shape[-2:]) != (Hs, Ws), "the shape is meant to be reflect-padded"
    pad = torch.ones(pre.shape, dtype=torch.bool)
    pad[..., :Hs, :Ws] = False
    clamped = ((pre < 0) | (pre > 1)).cpu()
    lo, hi = Wv.FILTERS[WAVE[0]]
    want_loss, want, _, smallest = Wv.value_and_grad(pre[..., :Hs, :Ws].cpu(), hr.cpu(), 1.0, True, LAM / hr.numel(), lo, hi, WAVE[1])
    assert float(want.abs().max()) > 0
    l1, out = torch.full((1,), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    # the term alone (an L1 seed of weight 0)
    gpre.fill_(NAN)
    assert _pixel(lib, plan, hr, l1, weight=0.0) == 0 and _wavelet(lib, plan, hr, out) == 0
    got = gpre.view(pre.shape).double().cpu()
    assert bool(torch.isfinite(got).all()), dtype
    assert int(torch.count_nonzero(got[pad])) == 0, f"{dtype}: seed in the padding"
    assert int(torch.count_nonzero(got[clamped])) == 0, f"{dtype}: seed where the clamp is active"
    nbad, worst = _gate(got[..., :Hs, :Ws], want)
    print(f"{dtype}: wavelet seed, largest |got - ref| / bound {worst:.3f}; value {float(out):.9e} against {want_loss:.9e}; "
          f"smallest non-zero |c| {smallest:.3g}")
    assert nbad == 0, f"{dtype}: {nbad} seed elements beyond the gate, worst ratio {worst:.3f}"
    assert abs(float(out) - want_loss) <= 1.2e-7 * abs(want_loss), (dtype, float(out), want_loss)
    # behind the L1 seed
    gpre.fill_(NAN)
    _lib.check(lib.m2t_l1_loss(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(l1), _lib.ptr(plan.workspace),
                               _lib.stream_ptr()), "m2t_l1_loss")
    assert _wavelet(lib, plan, hr, out) == 0
    got = gpre.view(pre.shape).double().cpu()
    inner = pre[..., :Hs, :Ws].double().cpu()
    d = inner.clamp(0.0, 1.0) - hr.double().cpu()
    seed_l1 = RP.derivative("l1", d) * RP.clamp_mask(inner) * float(torch.tensor(1.0 / hr.numel(), dtype=torch.float32))
    nbad, worst = _gate(got[..., :Hs, :Ws], want, prefill=seed_l1)
    assert nbad == 0, f"{dtype}: {nbad} elements of L1 + wavelet beyond the gate, worst ratio {worst:.3f}"
    assert int(torch.count_nonzero(got[pad])) == 0 and int(torch.count_nonzero(got[clamped])) == 0, dtype


def test_plan_entry_state_and_argument_errors():
    """State rules of m2t_ssim_loss; the argument refusals come before any launch."""
    _lib, lib = _lib_()
    model = _model(2, "fp32", NB)
    x, hr = _pair(2, "fp32", 1, 20, 28)
    plan = model._plan_for(x)
    out = torch.zeros(1, device="cuda")
    assert _wavelet(lib, plan, hr, out) == STATE                     # before a forward
    _forward(lib, model, plan, x)
    assert _wavelet(lib, plan, hr, out) == STATE                     # before any seed
    assert _pixel(lib, plan, hr, out, deferred=True) == 0
    assert _wavelet(lib, plan, hr, out) == STATE                     # a deferred request leaves no materialised seed
    assert b"materialised" in lib.m2t_last_error_string()
    assert _pixel(lib, plan, hr, out) == 0
    seed = plan.ws_tensor("gpre", dtype=torch.float32).clone()
    scratch = _scratch(lib, 1, 3, 40, 56, 3, 8)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    good = _args(*WAVE)
    import ctypes as C
    arr = lambda v: (C.c_double * len(v))(*v)
    for bad in (dict(hr=None), dict(out=None), dict(scratch=None), dict(ws=None), dict(R=0.0), dict(R=float("inf")), dict(div=0.0),
                dict(div=NAN), dict(w=NAN), dict(lo=None), dict(hi=None), dict(taps=1), dict(taps=9), dict(J=0), dict(J=4),
                dict(eps=-1.0), dict(eps=NAN), dict(bw=arr([0.0] * 7)), dict(bw=arr([1.0, -1.0, 1, 1, 1, 1, 0])),
                dict(lo=arr([NAN] * 4))):
        a = dict(hr=_lib.ptr(hr), out=_lib.ptr(out), scratch=_lib.ptr(scratch), ws=ws, R=1.0, div=1.0, w=LAM, lo=good[0], hi=good[1],
                 taps=good[2], J=good[3], bw=None, eps=0.0)
        a.update(bad)
        assert lib.m2t_wavelet_loss(plan.handle, a["hr"], a["w"], a["div"], a["R"], a["lo"], a["hi"], a["taps"], a["J"], a["bw"], a["eps"],
                                    a["out"], 0, a["scratch"], a["ws"], st) == ARG, bad
    assert lib.m2t_wavelet_loss(None, _lib.ptr(hr), LAM, 1.0, 1.0, *good, _lib.ptr(out), 0, _lib.ptr(scratch), ws, st) == ARG
    torch.cuda.synchronize()
    assert torch.equal(plan.ws_tensor("gpre", dtype=torch.float32), seed)        # a refused call touches nothing
    assert _wavelet(lib, plan, hr, out) == 0 and float(out) > 0


# ------------------------------------------------------------------ 5. TrainStep against the sequence by hand
def _by_hand(model, plan, x, hr, lam=LAM, pix_div=None, wav_div=None, args=None):
    """(l1 [1], wavelet [1], gradients): m2t_forward -> m2t_pixel_loss (l1) -> m2t_wavelet_loss -> m2t_backward into fresh buffers."""
    _lib, lib = _lib_()
    l1, wv = torch.full((1,), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    grads = torch.full_like(model.flat_params, NAN)
    _forward(lib, model, plan, x)
    assert _pixel(lib, plan, hr, l1, divisor=pix_div) == 0
    assert _wavelet(lib, plan, hr, wv, weight=lam, divisor=wav_div, args=args) == 0
    _backward(lib, model, plan, x, grads)
    torch.cuda.synchronize()
    return l1, wv, grads


@pytest.mark.parametrize("dtype,scale,kw", [("bf16", 4, dict(wavelet="db2", wavelet_levels=2)),
                                            ("fp32", 2, dict(wavelet="haar", wavelet_levels=3, wavelet_band_weights=[1.0] * 9 + [0.5],
                                                             wavelet_eps=1e-3))], ids=["bf16-x4-db2", "fp32-x2-haar3-LL-eps"])
def test_train_step_is_the_sequence_by_hand(dtype, scale, kw):
    """Two steps with different batches at (2, 20, 28): loss, gradients, parameters and moments bit-identical to m2t_forward ->
    m2t_pixel_loss -> m2t_wavelet_loss -> m2t_backward -> m2t_adam_step on a twin; the term is live."""
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    B, H, W = 2, 20, 28
    m_a, m_b = _model(scale, dtype, NB), _model(scale, dtype, NB)
    ts = TrainStep(m_a, lr=1e-4, world_size=1, lambda_wavelet=LAM, **kw)
    args = _args(kw["wavelet"], kw["wavelet_levels"], kw.get("wavelet_band_weights"), kw.get("wavelet_eps", 0.0))
    exp_avg, exp_avg_sq = torch.zeros_like(m_b.flat_params), torch.zeros_like(m_b.flat_params)
    first_grads = None
    for step in range(2):
        x, hr = _pair(scale, dtype, B, H, W, step)
        loss = ts.step(x, hr)
        torch.cuda.synchronize()
        plan = m_b._plan_for(x)
        l1, wv, grads = _by_hand(m_b, plan, x, hr, args=args)
        if step == 0:
            first_grads = grads.clone()
        n = grads.numel()
        _lib.check(lib.m2t_adam_step(_lib.ptr(m_b.flat_params), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), n, 1e-4, 0.9,
                                     0.999, 1e-8, step + 1, 1.0, _lib.stream_ptr()), "m2t_adam_step")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(grads).all()) and float(wv) > 0 and float(l1) > 0
        assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.wavelet_loss, wv) and torch.equal(loss, l1 + wv), (step, float(loss))
        assert ts.loss is loss
        assert list(ts._wavelet_scratch) == [(B, H * scale, W * scale, args[3], args[2])]          # cached per shape
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


def test_lambda_wavelet_zero_is_the_default_step_bit_for_bit():
    from m2trans_amd.train_step import TrainStep
    scale, dtype, B, H, W = 4, "bf16", 2, 20, 28
    res = []
    for kw in ({}, {"lambda_wavelet": 0.0, "wavelet": "db2", "wavelet_levels": 3}):
        model = _model(scale, dtype, NB)
        ts = TrainStep(model, lr=1e-4, world_size=1, **kw)
        assert ts.wavelet_loss is None and ts._wavelet_scratch == {}
        out = []
        for step in range(2):
            x, hr = _pair(scale, dtype, B, H, W, step)
            loss = ts.step(x, hr)
            torch.cuda.synchronize()
            assert ts.wavelet_loss is None and loss is ts.l1_loss and ts._wavelet_scratch == {}
            out.append((loss.clone(), ts.grads.clone(), model.flat_params.detach().clone()))
        res.append((model, out))
    (model, a), (_, b) = res
    for step in range(2):
        assert torch.equal(a[step][0], b[step][0])
        assert_flat_equal(model, a[step][1], b[step][1], f"gradients, step {step}")
        assert_flat_equal(model, a[step][2], b[step][2], f"parameters, step {step}")


def test_accumulated_wavelet_equals_the_micro_batch_gradients_summed_in_call_order():
    """accum_steps = 2 at micro-batch (1, 20, 28), bf16 x4: the accumulated buffer is the fp32 sum, in call order, of the two
    micro-batch gradients taken by hand with the cycle's divisor (the global number of coefficients per band: 2 x 3 x 80 x 112);
    ts.wavelet_loss is the sum of the two."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    x, hr = _pair(4, "bf16", 2, 20, 28)
    m_a, m_b = _model(4, "bf16", NB), _model(4, "bf16", NB)
    ts = TrainStep(m_a, world_size=1, accum_steps=2, lambda_wavelet=LAM, wavelet=WAVE[0], wavelet_levels=WAVE[1])
    ts.forward_backward(x[0:1], hr[0:1])
    with pytest.raises(M2TError):
        ts.optimizer_step()                                          # in mid-cycle
    with pytest.raises(M2TError):
        ts.set_lambda_wavelet(0.0)
    loss = ts.forward_backward(x[1:2], hr[1:2])
    torch.cuda.synchronize()
    parts = []
    for i in range(2):
        cx, chr_ = x[i:i + 1].contiguous(), hr[i:i + 1].contiguous()
        parts.append(_by_hand(m_b, m_b._plan_for(cx), cx, chr_, pix_div=hr.numel(), wav_div=hr.numel()))
    assert float(parts[1][2].abs().max()) > 0 and float(parts[1][1]) > 0
    assert torch.equal(ts.wavelet_loss, parts[0][1] + parts[1][1]), (float(ts.wavelet_loss), float(parts[0][1] + parts[1][1]))
    assert torch.equal(ts.l1_loss, parts[0][0] + parts[1][0])
    assert torch.equal(loss, ts.l1_loss + ts.wavelet_loss)
    assert_flat_equal(m_a, ts.grads, parts[0][2] + parts[1][2], "accumulated L1 + wavelet")
    ts.optimizer_step()
    assert ts.micro_count == 0


def test_all_terms_together_add_their_seeds():
    """TrainStep with every optional term issues pixel -> SSIM -> MS-SSIM -> FFT -> VIF -> GMSD -> wavelet -> backward: bit-identical
    to that sequence by hand; and the seed after the seven contributions against the one without the wavelet term plus the wavelet term
    alone: one fp32 add within half an ulp of its sum.  48 x 48 at x4: 192 x 192 suits the transform and the five levels."""
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    scale, dtype, B, H, W = 4, "bf16", 1, 48, 48
    x, hr = _pair(scale, dtype, B, H, W)
    Hs = Ws = 192
    lam_s, lam_m, lam_f, lam_v, lam_g = 0.1, 0.16, 0.05, 0.1, 0.05
    m_a, m_b = _model(scale, dtype, NB), _model(scale, dtype, NB)
    ts = TrainStep(m_a, world_size=1, lambda_ssim=lam_s, lambda_msssim=lam_m, lambda_fft=lam_f, lambda_vif=lam_v, lambda_gmsd=lam_g,
                   lambda_wavelet=LAM, wavelet=WAVE[0], wavelet_levels=WAVE[1])
    loss = ts.forward_backward(x, hr)
    torch.cuda.synchronize()
    plan = m_b._plan_for(x)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    l1, ss, ms, ff, vf, gm, wv = (torch.full((1,), NAN, device="cuda") for _ in range(7))
    s_ssim = torch.empty(lib.m2t_ssim_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    s_ms = torch.empty(lib.m2t_msssim_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    s_fft = torch.empty(lib.m2t_fft_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    s_vif = torch.empty(lib.m2t_vif_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    s_gmsd = torch.empty(lib.m2t_gmsd_loss_scratch_bytes(B, 3, Hs, Ws), dtype=torch.uint8, device="cuda")
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    _forward(lib, m_b, plan, x)

    def seed(pixel_weight, others, with_wavelet):
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
            _lib.check(lib.m2t_gmsd_loss(plan.handle, _lib.ptr(hr), lam_g, float(B), 1.0, _lib.ptr(gm), 0, _lib.ptr(s_gmsd), ws, st),
                       "m2t_gmsd_loss")
        if with_wavelet:
            assert _wavelet(lib, plan, hr, wv) == 0
        torch.cuda.synchronize()
        return gpre.clone()

    before, alone = seed(1.0, True, False).double().cpu(), seed(0.0, False, True).double().cpu()
    assert bool(torch.isfinite(alone).all()) and float(alone.abs().max()) > 0
    full = seed(1.0, True, True).double().cpu()
    excess = (full - (before + alone)).abs() - HALF_ULP * (before + alone).abs()
    assert float(excess.max()) <= 0.0, float(excess.max())
    g_b = torch.full_like(m_b.flat_params, NAN)
    _backward(lib, m_b, plan, x, g_b)
    torch.cuda.synchronize()
    assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.ssim_loss, ss) and torch.equal(ts.msssim_loss, ms) and torch.equal(ts.fft_loss, ff)
    assert torch.equal(ts.vif_loss, vf) and torch.equal(ts.gmsd_loss, gm) and torch.equal(ts.wavelet_loss, wv)
    assert torch.equal(loss, ts.l1_loss + ts.ssim_loss + ts.msssim_loss + ts.fft_loss + ts.vif_loss + ts.gmsd_loss + ts.wavelet_loss)
    assert_flat_equal(m_a, ts.grads, g_b, "pixel + SSIM + MS-SSIM + FFT + VIF + GMSD + wavelet")


# ------------------------------------------------------------------ 6. the autograd Function
def test_wavelet_loss_function_gives_the_restatements_gradient():
    from m2trans_amd.losses import WaveletLoss, wavelet_loss
    shape = (2, 3, 33, 70)
    lo, hi = Wv.DB2
    x, y = Wv.mixed_pair(shape, seed=21)
    want_loss, want, _, _ = Wv.value_and_grad(x, y, 1.0, False, None, lo, hi, 2)
    leaf = x.cuda().requires_grad_(True)
    got = wavelet_loss(leaf, y.cuda(), 1.0, "db2", 2)
    (got * 3.0).backward()                                          # (an upstream factor reaches the gradient)
    torch.cuda.synchronize()
    assert got.shape == () and abs(float(got.detach()) - want_loss) <= 1.2e-7 * abs(want_loss)
    assert bool(torch.isfinite(leaf.grad).all())
    nbad, worst = _gate(leaf.grad.double().cpu() / 3.0, want)
    print(f"wavelet_loss Function: largest |got - ref| / bound {worst:.3f}")
    # (the division by 3 undoes an fp32 product: one more rounding on each side of it, 1.2e-7 |ref| -- inside the 1e-6 |ref| term)
    assert nbad == 0, (nbad, worst)
    assert float(WaveletLoss(1.0, "db2", 2)(x.cuda(), y.cuda())) == float(got.detach())
    w = [1.0] * 9 + [0.5]
    w255 = Wv.value_and_grad(x * 255.0, y * 255.0, 255.0, False, None, Wv.HAAR[0], Wv.HAAR[1], 3, w, 1e-3)[0]
    assert abs(float(WaveletLoss(255.0, "haar", 3, w, 1e-3)(x.cuda() * 255.0, y.cuda() * 255.0)) - w255) <= 1.2e-7 * abs(w255)
