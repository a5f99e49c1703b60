"""GPU tests of the VGG19 feature loss (losses.PerceptualLoss, m2t_vgg_* of include/m2t_perceptual.h; k_vgg.hip, m2t_vgg.hip).

Random He-initialised weights (none ship).  Operators are gated elementwise against fp64 on identical bf16 inputs; the loss value and the
input gradient are TEACHER-FORCED (tests/vgg_ref.py): the fp64 reference takes masks, arg-maxes and signs from the activations the
device itself saved, and the budget is MARGIN x the error of the bf16 emulation on the same masks -- never a figure from a HIP run."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import vgg_ref as V

pytestmark = pytest.mark.gpu

SD = V.random_weights(11)


@pytest.fixture(scope="module")
def lib():
    from m2trans_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def tower():
    from m2trans_amd.losses import PerceptualLoss
    return PerceptualLoss(device="cuda").load_vgg_state_dict(SD)


def _nhwc(t):
    """[N,C,H,W] float -> bf16 NHWC on the device"""
    return t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()


def _nchw(t):
    """bf16 NHWC on the device -> [N,C,H,W] float64 on the host"""
    return t.permute(0, 3, 1, 2).double().cpu()


def _rand_bf16(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).float()


def _sync_check(lib, rc, what):
    from m2trans_amd import _lib
    _lib.check(rc, what)
    torch.cuda.synchronize()


def _w(l):
    return V.bf16(SD[f"features.{V.LAYERS[l]}.weight"]), SD[f"features.{V.LAYERS[l]}.bias"].double()


# ------------------------------------------------------------------------------------------------------------- 1. convolution
@pytest.mark.parametrize("layer,N,H,W", [(1, 2, 9, 19), (4, 1, 8, 8), (9, 1, 5, 7), (4, 1, 3, 3)],
                         ids=["64-64@2x9x19", "128-256@8x8", "512-512@5x7", "256-128@3x3"])
def test_convolution_forward_and_data_gradient_against_fp64(lib, tower, layer, N, H, W):
    """|err| <= 2^-8 |ref| + 2 K 2^-24 (|a| (*) |w| + |b|), K = 9 Cin: one bf16 ulp of the output plus the fp32 accumulation bound.  The
    forward of layer l is Cin_l -> Cout_l; its data gradient is the same kernel at Cout_l -> Cin_l (256 -> 128 for layer 4)."""
    from m2trans_amd import _lib
    ci, co = V.CIN[layer], V.COUT[layer]
    w, b = _w(layer)
    a = _rand_bf16((N, ci, H, W), 1)
    out = torch.full((N, H, W, co), float("nan"), dtype=torch.bfloat16, device="cuda")
    ad = _nhwc(a)
    _sync_check(lib, lib.m2t_vgg_conv_forward(tower.handle, layer, _lib.ptr(ad), _lib.ptr(out), N, H, W, 1.0, _lib.stream_ptr()), "conv_forward")
    ref = F.relu(F.conv2d(a.double(), w, b, padding=1))
    pre_bound = V.conv_bound(a.double(), w, b, 9 * ci)
    worst = V.conv_gate(_nchw(out), ref, pre_bound)
    print(f"layer {layer} forward {ci}->{co} at {N}x{H}x{W}: worst ratio to the gate {worst:.3f}")
    assert worst <= 1.0
    assert float(ref.max()) > 0 and float((ref == 0).double().mean()) > 0.1          # both sides of the ReLU are present

    g = _rand_bf16((N, co, H, W), 2)
    gd = _nhwc(g)
    wt = w.transpose(0, 1).flip(2, 3)
    gref = F.conv2d(g.double(), wt, padding=1)
    gbound = V.conv_bound(g.double(), wt, None, 9 * co)
    for masked in (False, True):
        gin = torch.full((N, H, W, ci), float("nan"), dtype=torch.bfloat16, device="cuda")
        _sync_check(lib, lib.m2t_vgg_conv_backward(tower.handle, layer, _lib.ptr(gd), _lib.ptr(ad) if masked else None, _lib.ptr(gin),
                                                   N, H, W, 1.0, _lib.stream_ptr()), "conv_backward")
        r = gref * (a.double() > 0) if masked else gref
        worst = V.conv_gate(_nchw(gin), r, gbound)
        print(f"layer {layer} data gradient {co}->{ci} (mask {masked}): worst ratio {worst:.3f}")
        assert worst <= 1.0
        if masked:
            assert int(torch.count_nonzero(_nchw(gin)[a <= 0])) == 0


def test_first_layer_forward_and_its_64_to_3_gradient_against_fp64(lib, tower):
    from m2trans_amd import _lib
    N, H, W = 1, 17, 33
    w, b = _w(0)
    g0 = torch.Generator().manual_seed(3)
    x = torch.rand(N, 3, H, W, generator=g0).to(torch.bfloat16).float()
    a = V.normalise(x, 1.0, False, True)                                  # fp32 operations, as the kernel's: identical inputs to the sum
    out = torch.full((N, H, W, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    xd = x.cuda()
    _sync_check(lib, lib.m2t_vgg_conv_forward(tower.handle, 0, _lib.ptr(xd), _lib.ptr(out), N, H, W, 1.0, _lib.stream_ptr()), "conv_forward 0")
    ref = F.relu(F.conv2d(a, w, b, padding=1))
    worst = V.conv_gate(_nchw(out), ref, V.conv_bound(a, w, b, 27))
    print(f"conv1_1 forward: worst ratio {worst:.3f}")
    assert worst <= 1.0

    g = _rand_bf16((N, 64, H, W), 4)
    gd = _nhwc(g)
    wt = w.transpose(0, 1).flip(2, 3)
    std = torch.tensor(V.STD, dtype=torch.float64).view(1, 3, 1, 1)
    for R in (1.0, 255.0):
        gin = torch.zeros(N, 3, H, W, dtype=torch.float32, device="cuda")
        _sync_check(lib, lib.m2t_vgg_conv_backward(tower.handle, 0, _lib.ptr(gd), None, _lib.ptr(gin), N, H, W, R, _lib.stream_ptr()), "conv_backward 0")
        gref = F.conv2d(g.double(), wt, padding=1) / (std * R)
        # an fp32 output: the bf16 ulp of the gate gives way to the roundings of std * R and of the division (2 x 2^-24, taken as 2^-22)
        bound = V.conv_bound(g.double(), wt, None, 9 * 64) / (std * R)
        worst = float(((gin.double().cpu() - gref).abs() / (2.0 ** -22 * gref.abs() + bound)).max())
        print(f"conv1_1 data gradient, R = {R}: worst ratio {worst:.3f}")
        assert worst <= 1.0 and float(gref.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------- 2. pool
@pytest.mark.parametrize("C_", [8, 64])
def test_pool_forward_and_backward_equal_torch_exactly(lib, C_):
    from m2trans_amd import _lib
    g = torch.Generator().manual_seed(5)
    a = (torch.randint(-2, 3, (2, C_, 5, 7), generator=g).float() * 0.5).requires_grad_(True)      # odd sizes, many ties, zeros, negatives
    go = _rand_bf16((2, C_, 2, 3), 6)
    ref = F.max_pool2d(a, 2)
    ref.backward(go)
    out = torch.full((2, 2, 3, C_), float("nan"), dtype=torch.bfloat16, device="cuda")
    ad, god = _nhwc(a.detach()), _nhwc(go)                  # kept alive: a temporary's block would be handed to the next one
    _sync_check(lib, lib.m2t_vgg_pool_forward(_lib.ptr(ad), _lib.ptr(out), 2, 5, 7, C_, _lib.stream_ptr()), "pool_forward")
    assert torch.equal(_nchw(out), ref.detach().double())
    for relu in (0, 1):
        gin = torch.full((2, 5, 7, C_), float("nan"), dtype=torch.bfloat16, device="cuda")
        _sync_check(lib, lib.m2t_vgg_pool_backward(_lib.ptr(ad), _lib.ptr(god), _lib.ptr(gin), 2, 5, 7, C_, relu,
                                                   _lib.stream_ptr()), "pool_backward")
        want = a.grad.double() * (a.detach() > 0) if relu else a.grad.double()
        assert torch.equal(_nchw(gin), want)
        assert int(torch.count_nonzero(_nchw(gin)[:, :, 4, :])) == 0 and int(torch.count_nonzero(_nchw(gin)[:, :, :, 6])) == 0


# ------------------------------------------------------------------------------------------------------------- 3 - 5. the loss
def _pair(shape, seed, R=1.0, spill=0.0):
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(shape, generator=g) * R
    x = y + 0.1 * R * torch.randn(shape, generator=g)
    if spill:
        x = x + spill * R * (torch.rand(shape, generator=g) - 0.5)
    return x.float(), y.float()


def _run(lib, tower, x, y, R=1.0, clamp=0, crit="l1", tw=(1.0,) * 5, scale=1.0, gx=None, ws=None, per=None, acc=0, loss=None):
    """one m2t_vgg_loss_tensor call on device tensors (x may be a strided view; gx has x's strides); returns (loss [1], workspace)"""
    from m2trans_amd import _lib
    B, Cn, H, W = x.shape
    assert x.stride(3) == 1 and x.stride(1) * Cn == x.stride(0) and (gx is None or gx.stride() == x.stride())
    if ws is None:
        ws = torch.empty(lib.m2t_vgg_workspace_bytes(B, H, W, 1 if gx is not None else 0), dtype=torch.uint8, device="cuda")
    if loss is None:
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    kind, param = V.KINDS[crit]
    _sync_check(lib, lib.m2t_vgg_loss_tensor(tower.handle, _lib.ptr(x), _lib.ptr(y), B, Cn, H, W, x.stride(0), x.stride(2), R, clamp, kind, param,
                                             (C.c_double * 5)(*tw), scale, _lib.ptr(gx), _lib.ptr(loss), _lib.ptr(per), acc, _lib.ptr(ws),
                                             _lib.stream_ptr()), "m2t_vgg_loss_tensor")
    return loss, ws


def _region(lib, ws, B, H, W, region, index, layer):
    lv, c = V.LEVEL[layer], V.COUT[layer]
    h, w = H >> lv, W >> lv
    off = lib.m2t_vgg_workspace_offset(B, H, W, region, index)
    n = B * h * w * c
    return _nchw(ws[off:off + 2 * n].view(torch.bfloat16).view(B, h, w, c))


def _saved(lib, ws, B, H, W):
    acts = [_region(lib, ws, B, H, W, 0, l, l) for l in range(13)]
    ytaps = [_region(lib, ws, B, H, W, 1, k, V.TAP_LAYERS[k]) for k in range(5)]
    return acts, ytaps


@pytest.mark.parametrize("crit", ["l1", "sl1", "l2"])
def test_loss_value_from_the_stored_taps_and_taps_against_fp64(lib, tower, crit):
    shape, tw, scale = (2, 3, 40, 48), (1.0, 0.5, 0.0, 2.0, 1.5), 0.7
    x, y = _pair(shape, 21)
    per = torch.full((5,), float("nan"), dtype=torch.float64, device="cuda")
    loss, ws = _run(lib, tower, x.cuda(), y.cuda(), crit=crit, tw=tw, scale=scale, per=per)
    acts, ytaps = _saved(lib, ws, *shape[:1], *shape[2:])
    want, means = V.loss_from_taps([acts[l] for l in V.TAP_LAYERS], ytaps, tw, crit, scale)
    got = float(loss.cpu())
    print(f"{crit}: device {got:.9g}, fp64 from the stored taps {float(want):.9g}")
    assert abs(got - float(want)) <= 1e-6 * abs(float(want))                      # the fp32 rounding of an fp64 sum
    for k in range(5):
        assert abs(float(per[k].cpu()) - float(means[k])) <= 1e-6 * float(means[k])
    # accumulate adds to what is there
    loss2, _ = _run(lib, tower, x.cuda(), y.cuda(), crit=crit, tw=tw, scale=scale, ws=ws, acc=1, loss=torch.full((1,), 2.0, device="cuda"))
    assert abs(float(loss2.cpu()) - (2.0 + got)) <= 2e-7 * (2.0 + got)
    if crit != "l1":
        return
    # the stored taps against the exact fp64 forward: within MARGIN x the emulation's own error, tap by tap, for both halves
    for src, dev in ((x, [acts[l] for l in V.TAP_LAYERS]), (y, ytaps)):
        exact, emul = V.forward_exact(src, SD), V.forward_emulated(src, SD)
        for k, l in enumerate(V.TAP_LAYERS):
            err, budget = float((dev[k] - exact[l]).abs().max()), V.MARGIN * float((emul[l] - exact[l]).abs().max())
            print(f"  tap {k}: device {err:.3e}, budget {budget:.3e}")
            assert err <= budget, (k, err, budget)


GRAD_CASES = {
    "2x3x40x48-l1": dict(shape=(2, 3, 40, 48), crit="l1"),
    "1x3x16x16-sl1": dict(shape=(1, 3, 16, 16), crit="sl1"),
    "1x1x33x47-l2-clamp-255": dict(shape=(1, 1, 33, 47), crit="l2", R=255.0, clamp=1, spill=0.6),
    "2x3x40x48-strided-add-weights-clamp": dict(shape=(2, 3, 40, 48), crit="l1", clamp=1, spill=0.6, strided=True, prefill=True,
                                                tw=(0.3, 1.0, 0.0, 2.0, 0.5), scale=0.7),
    "1x3x17x31-sl1-add": dict(shape=(1, 3, 17, 31), crit="sl1", prefill=True, scale=50.0),
}


@pytest.mark.parametrize("case", list(GRAD_CASES), ids=list(GRAD_CASES))
def test_input_gradient_teacher_forced_from_the_saved_activations(lib, tower, case):
    c = dict(R=1.0, clamp=0, spill=0.0, strided=False, prefill=False, tw=(1.0,) * 5, scale=1.0)
    c.update(GRAD_CASES[case])
    B, Cn, H, W = c["shape"]
    x, y = _pair(c["shape"], 31, c["R"], c["spill"])
    g = torch.Generator().manual_seed(32)
    if c["strided"]:
        big = torch.full((B, Cn, H + 3, W + 5), float("nan"), device="cuda")
        xd = big[:, :, :H, :W]
        xd.copy_(x)
        gbig = torch.randn(B, Cn, H + 3, W + 5, generator=g).cuda()
        gx = gbig[:, :, :H, :W]
    else:
        xd = x.cuda()
        gbig = (torch.randn(c["shape"], generator=g) * 1e-3).cuda() if c["prefill"] else torch.zeros(c["shape"], device="cuda")
        gx = gbig
    before = gbig.clone()
    loss, ws = _run(lib, tower, xd, y.cuda(), R=c["R"], clamp=c["clamp"], crit=c["crit"], tw=c["tw"], scale=c["scale"], gx=gx)
    acts, ytaps = _saved(lib, ws, B, H, W)
    kw = dict(crit=c["crit"], tap_w=c["tw"], scale=c["scale"], R=c["R"], clamp=bool(c["clamp"]))
    exact = V.backward(acts, ytaps, SD, x, rounded=False, **kw)
    emul = V.backward(acts, ytaps, SD, x, rounded=True, **kw)
    got = (gx - before[:, :, :H, :W]).double().cpu() if c["strided"] else (gx - before).double().cpu()
    ok, err, budget = V.grad_gate(got, exact, emul)
    print(f"{case}: device {err:.3e} of the largest entry, budget {budget:.3e} (emulation {budget / V.MARGIN:.3e})")
    assert float(exact.abs().max()) > 0 and ok, (err, budget)
    if c["clamp"]:
        out = ((x < 0) | (x > c["R"]))
        assert int(out.sum()) > 0
        view = gx.cpu()
        assert torch.equal(view[out], before[:, :, :H, :W].cpu()[out] if c["strided"] else before.cpu()[out])      # untouched, bit for bit
    if c["strided"]:
        pad = torch.ones(B, Cn, H + 3, W + 5, dtype=torch.bool)
        pad[:, :, :H, :W] = False
        assert torch.equal(gbig.cpu()[pad], before.cpu()[pad])
    # the gradient regions of the workspace: the seed of relu5_1 is where the audit entry says
    g12 = _region(lib, ws, B, H, W, 3, 12, 12)
    seed = (c["scale"] * c["tw"][4] / acts[12].numel()) * V.rho_prime(acts[12] - ytaps[4], c["crit"]) * (acts[12] > 0)
    assert float((g12 - V.bf16(seed)).abs().max()) <= 2.0 ** -8 * float(seed.abs().max()) + 1e-300


def test_resize_goes_through_the_bicubic_resampler_and_back(lib, tower):
    from m2trans_amd.losses import PerceptualLoss
    p = PerceptualLoss(resize=True, device="cuda").load_vgg_state_dict(SD)
    shape = (1, 3, 40, 48)
    x, y = _pair(shape, 41)
    leaf = x.cuda().requires_grad_(True)
    loss = p(leaf, y.cuda())
    (2.0 * loss).backward()
    torch.cuda.synchronize()
    ws = p._ws[(1, 224, 224, True)]
    acts, ytaps = _saved(lib, ws, 1, 224, 224)
    want, _ = V.loss_from_taps([acts[l] for l in V.TAP_LAYERS], ytaps, (1.0,) * 5, "l1")
    assert abs(float(loss.detach()) - float(want)) <= 1e-6 * float(want)
    x224 = torch.zeros(1, 3, 224, 224)                       # the clamp is off: only the shape matters to the reference backward
    outs = []
    for rounded in (False, True):
        g224 = V.backward(acts, ytaps, SD, x224, rounded=rounded)
        t = x.double().clone().requires_grad_(True)
        F.interpolate(t, size=(224, 224), mode="bicubic", align_corners=True).backward(g224)
        outs.append(2.0 * t.grad)
    ok, err, budget = V.grad_gate(leaf.grad.double().cpu(), outs[0], outs[1])
    print(f"resize: device {err:.3e}, budget {budget:.3e}")
    assert ok, (err, budget)


def test_two_runs_are_bit_identical_and_a_poisoned_workspace_changes_no_bit(lib, tower):
    shape = (2, 3, 40, 48)
    x, y = _pair(shape, 51)
    xd, yd = x.cuda(), y.cuda()
    runs = []
    for fill in (0x00, 0xFF, 0x7F):                         # 0xFF.. / 0x7F7F are NaN patterns in bf16 and in fp64
        ws = torch.full((lib.m2t_vgg_workspace_bytes(2, 40, 48, 1),), fill, dtype=torch.uint8, device="cuda")
        gx = torch.zeros(shape, device="cuda")
        loss, _ = _run(lib, tower, xd, yd, crit="sl1", gx=gx, ws=ws)
        runs.append((loss.cpu(), gx.cpu()))
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all()) and float(runs[0][1].abs().max()) > 0
    for l, g in runs[1:]:
        assert torch.equal(l.view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(g.view(torch.int32), runs[0][1].view(torch.int32))
    # value only: the same loss bits, no gradient launches (a smaller workspace suffices)
    loss, _ = _run(lib, tower, xd, yd, crit="sl1")
    assert torch.equal(loss.cpu().view(torch.int32), runs[0][0].view(torch.int32))


def test_module_matches_the_plan_free_entry_and_autograd_scales(lib, tower):
    shape = (1, 1, 24, 40)
    x, y = _pair(shape, 61)
    leaf = x.cuda().requires_grad_(True)
    loss = tower(leaf, y.cuda())
    (3.0 * loss).backward()
    gx = torch.zeros(shape, device="cuda")
    ref, _ = _run(lib, tower, x.cuda(), y.cuda(), gx=gx)
    assert torch.equal(loss.detach().cpu().view(1), ref.cpu()) and torch.equal(leaf.grad.cpu(), (gx * 3.0).cpu())
    with torch.no_grad():
        assert torch.equal(tower(x.cuda(), y.cuda()).cpu().view(1), ref.cpu())


# ------------------------------------------------------------------------------------------------------------- 7. error paths
def test_error_paths_are_decided_before_any_launch(lib, tower):
    from m2trans_amd import _lib
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import PerceptualLoss
    x = torch.zeros(1, 3, 15, 32, device="cuda")
    with pytest.raises(M2TError, match="at least 16"):
        tower(x, x)
    loss = torch.full((1,), 5.0, device="cuda")
    tw = (C.c_double * 5)(1, 1, 1, 1, 1)
    one = torch.zeros(16, device="cuda")
    assert lib.m2t_vgg_loss_tensor(tower.handle, _lib.ptr(x), _lib.ptr(x), 1, 3, 15, 32, 3 * 15 * 32, 32, 1.0, 0, 0, 0.0, tw, 1.0, None,
                                   _lib.ptr(loss), None, 0, _lib.ptr(one), _lib.stream_ptr()) == -2
    fresh = PerceptualLoss(device="cuda")
    x = torch.zeros(1, 3, 32, 32, device="cuda")
    with pytest.raises(M2TError, match="no VGG19 weights loaded"):
        fresh(x, x)
    assert lib.m2t_vgg_loss_tensor(fresh.handle, _lib.ptr(x), _lib.ptr(x), 1, 3, 32, 32, 3 * 32 * 32, 32, 1.0, 0, 0, 0.0, tw, 1.0, None,
                                   _lib.ptr(loss), None, 0, _lib.ptr(one), _lib.stream_ptr()) == -3
    h = C.c_void_p()
    assert lib.m2t_vgg_create(C.byref(h), _lib.F32) == -2 and b"bf16 only" in lib.m2t_last_error_string()
    torch.cuda.synchronize()
    assert float(loss.cpu()) == 5.0                         # nothing was launched


# ------------------------------------------------------------------------------------------------------------- 6. TrainStep
LAM = 0.05
TS_TW = [1.0, 0.5, 0.25, 2.0, 1.5]


def _ts_parts():
    from tests.test_gpu_msssim_loss import _pixel
    from tests.test_gpu_pixel_loss import _backward, _forward, _images, _model, _srpre
    return _pixel, _backward, _forward, _images, _model, _srpre


@pytest.fixture(scope="module")
def ts_tower():
    from m2trans_amd.losses import PerceptualLoss
    return PerceptualLoss(weights=TS_TW, criterion="sl1", device="cuda").load_vgg_state_dict(SD)


def _vgg(lib, plan, tower, hr, out, weight=LAM, divisor=None, accumulate=0):
    from m2trans_amd import _lib
    B, _, Hs, Ws = hr.shape
    rc = lib.m2t_vgg_loss(plan.handle, tower.handle, _lib.ptr(hr), weight, float(B if divisor is None else divisor), 1.0, tower.kind, tower.param,
                          tower.tap_weights(), _lib.ptr(out), accumulate, _lib.ptr(tower.workspace(B, Hs, Ws, True)), _lib.ptr(plan.workspace),
                          _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _by_hand(lib, model, plan, tower, x, hr, pix_div=None, vgg_div=None):
    """(l1 [1], term [1], gradients): m2t_forward -> m2t_pixel_loss (l1) -> m2t_vgg_loss -> m2t_backward into fresh buffers."""
    _pixel, _backward, _forward, _, _, _ = _ts_parts()
    l1, pv = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    grads = torch.full_like(model.flat_params, float("nan"))
    _forward(lib, model, plan, x)
    assert _pixel(lib, plan, hr, l1, divisor=pix_div) == 0
    assert _vgg(lib, plan, tower, hr, pv, divisor=vgg_div) == 0
    _backward(lib, model, plan, x, grads)
    torch.cuda.synchronize()
    return l1, pv, grads


def test_plan_entry_adds_the_plan_free_gradient_into_the_seed_bit_for_bit(lib, ts_tower):
    """x2, nf 64, one block, LR 24 x 24, B = 2: the seed after m2t_vgg_loss is the seed before it with the plan-free gradient of the same
    pre-clamp output added, bit for bit; nothing lands in the reflect padding or where the clamp is active; the state rules."""
    _pixel, _backward, _forward, _images, _model, _srpre = _ts_parts()
    B, H, W, scale = 2, 24, 24, 2
    model = _model(scale, "bf16", 1)
    x, hr = _images(B, H, W, scale)
    plan = model._plan_for(x)
    out = torch.full((1,), float("nan"), device="cuda")
    assert _vgg(lib, plan, ts_tower, hr, out) == -3                      # before a forward
    _forward(lib, model, plan, x)
    assert _vgg(lib, plan, ts_tower, hr, out) == -3                      # before any seed
    assert _pixel(lib, plan, hr, out, deferred=True) == 0
    assert _vgg(lib, plan, ts_tower, hr, out) == -3 and b"materialised" in lib.m2t_last_error_string()      # after a deferred pixel loss
    l1 = torch.full((1,), float("nan"), device="cuda")
    assert _pixel(lib, plan, hr, l1) == 0
    torch.cuda.synchronize()
    Hs, Ws = H * scale, W * scale
    pre = _srpre(plan, B, scale)
    gpre = plan.ws_tensor("gpre", dtype=torch.float32).view(pre.shape)
    before = gpre.clone()
    assert _vgg(lib, plan, ts_tower, hr, out) == 0
    after = gpre.clone()
    want = before.clone()
    lam32 = float(torch.tensor(LAM, dtype=torch.float32))                # the plan entry takes its weight as a float
    ref, _ = _run(lib, ts_tower, pre[:, :, :Hs, :Ws], hr, clamp=1, crit="sl1", tw=TS_TW, scale=lam32, gx=want[:, :, :Hs, :Ws])
    assert torch.equal(after.view(torch.int32), want.view(torch.int32)) and not torch.equal(after, before)
    assert torch.equal(out.cpu(), ref.cpu()) and float(out) > 0
    pad = torch.ones(pre.shape, dtype=torch.bool)
    pad[..., :Hs, :Ws] = False
    assert torch.equal(after.cpu()[pad], before.cpu()[pad])
    clamped = ((pre < 0) | (pre > 1)).cpu()
    assert torch.equal(after.cpu()[clamped], before.cpu()[clamped])
    # accumulate adds the value
    acc = torch.full((1,), 2.0, device="cuda")
    assert _vgg(lib, plan, ts_tower, hr, acc, accumulate=1) == 0
    assert abs(float(acc) - (2.0 + float(out))) <= 2e-7 * (2.0 + float(out))


def test_train_step_total_default_step_accumulation_and_checkpoint(lib, ts_tower):
    from m2trans_amd._lib import M2TError
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    from m2trans_amd.losses import PerceptualLoss
    from m2trans_amd.train_step import TrainStep
    from tests.gpu_util import assert_flat_equal
    _pixel, _backward, _forward, _images, _model, _srpre = _ts_parts()
    B, H, W, scale = 2, 24, 24, 2
    x, hr = _images(B, H, W, scale)
    # the step is the sequence by hand: total = pixel term + the term; gradients bit for bit
    m_a, m_b = _model(scale, "bf16", 1), _model(scale, "bf16", 1)
    ts = TrainStep(m_a, lr=1e-4, world_size=1, perceptual_loss=ts_tower, lambda_perceptual=LAM)
    loss = ts.forward_backward(x, hr)
    torch.cuda.synchronize()
    l1, pv, grads = _by_hand(lib, m_b, m_b._plan_for(x), ts_tower, x, hr)
    assert bool(torch.isfinite(grads).all()) and float(pv) > 0
    assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.perceptual_loss_value, pv) and torch.equal(loss, l1 + pv)
    assert_flat_equal(m_a, ts.grads, grads, "gradients")
    ts0 = TrainStep(_model(scale, "bf16", 1), world_size=1)
    ts0.forward_backward(x, hr)
    torch.cuda.synchronize()
    assert not torch.equal(ts0.grads, grads)                             # the term is live
    # lambda_perceptual = 0 is the default L1 step, bit for bit, after two steps
    res = []
    for kw in ({}, {"perceptual_loss": ts_tower, "lambda_perceptual": 0.0}):
        model = _model(scale, "bf16", 1)
        t = TrainStep(model, lr=1e-4, world_size=1, **kw)
        for step in range(2):
            lo = t.step(*_images(B, H, W, scale, step))
        torch.cuda.synchronize()
        assert t.perceptual_loss_value is None and lo is t.l1_loss
        res.append((model, lo.clone(), model.flat_params.detach().clone()))
    assert torch.equal(res[0][1], res[1][1])
    assert_flat_equal(res[0][0], res[0][2], res[1][2], "parameters after two steps")
    # accum_steps = 2: the fp32 sum, in call order, of the micro-batch gradients by hand with the cycle's divisors (the rule of the SSIM
    # term's accumulation test); the value is that of the joined batch
    m_c, m_d = _model(scale, "bf16", 1), _model(scale, "bf16", 1)
    ta = TrainStep(m_c, world_size=1, accum_steps=2, perceptual_loss=ts_tower, lambda_perceptual=LAM)
    ta.forward_backward(x[0:1], hr[0:1])
    with pytest.raises(M2TError):
        ta.set_lambda_perceptual(0.0)
    la = ta.forward_backward(x[1:2], hr[1:2])
    torch.cuda.synchronize()
    parts = []
    for i in range(2):
        cx, ch = x[i:i + 1].contiguous(), hr[i:i + 1].contiguous()
        parts.append(_by_hand(lib, m_d, m_d._plan_for(cx), ts_tower, cx, ch, pix_div=hr.numel(), vgg_div=2))
    assert torch.equal(ta.perceptual_loss_value, parts[0][1] + parts[1][1]) and torch.equal(ta.l1_loss, parts[0][0] + parts[1][0])
    assert torch.equal(la, ta.l1_loss + ta.perceptual_loss_value)
    assert_flat_equal(m_c, ta.grads, parts[0][2] + parts[1][2], "accumulated L1 + perceptual")
    assert abs(float(ta.perceptual_loss_value) - float(pv)) <= 1e-6 * float(pv)
    ta.optimizer_step()
    # a checkpoint round trip restores the settings (never the VGG19 weights)
    ck = export_checkpoint(m_a, ts, epoch=3)
    assert ck["m2t_loss"]["lambda_perceptual"] == LAM and ck["m2t_loss"]["perceptual_criterion"] == "sl1" and ck["m2t_loss"]["perceptual_weights"] == TS_TW
    other = PerceptualLoss(device="cuda").load_vgg_state_dict(SD)
    dst = TrainStep(_model(scale, "bf16", 1), world_size=1, perceptual_loss=other)
    import_checkpoint(ck, dst.model, dst)
    assert dst.lambda_perceptual == LAM and (other.criterion, other.kind, other.weights, other.resize) == ("sl1", 3, TS_TW, False)
    l2 = dst.forward_backward(x, hr)
    torch.cuda.synchronize()
    assert torch.equal(dst.perceptual_loss_value, pv)
    # a small SR image is refused by the step itself, on the host
    with pytest.raises(M2TError, match="at least 16"):
        TrainStep(_model(scale, "bf16", 1), world_size=1, perceptual_loss=ts_tower, lambda_perceptual=LAM)._perceptual_workspace_for(torch.zeros(1, 3, 12, 48))


def test_all_five_terms_accumulated_are_the_sequence_by_hand_bit_for_bit(lib, ts_tower):
    """Every optional term on at once, bf16 x4, accum_steps = 2, micro-batches (1, 3, 48, 48): 192 x 192 SR pixels, the smallest size
    that suits both the five MS-SSIM levels and the transform's 2^a 3^b rule.  The step issues pixel -> SSIM -> MS-SSIM -> FFT -> VIF ->
    perceptual -> backward per micro-batch; the six values and the accumulated gradients are those of that sequence issued by hand on a
    twin model with the cycle's divisors, summed in call order, and the total is the six values added in that order.  No tolerance."""
    from m2trans_amd import _lib
    from m2trans_amd.train_step import TrainStep
    from tests.gpu_util import assert_flat_equal
    from tests.test_gpu_msssim_loss import _model, _pair, _pixel
    from tests.test_gpu_pixel_loss import _backward, _forward
    scale, Hs, Ws = 4, 192, 192
    lam = {"ssim": 0.1, "msssim": 0.16, "fft": 0.05, "vif": 0.1}
    names = ["l1", "ssim", "msssim", "fft", "vif", "perceptual"]
    x, hr = _pair(scale, "bf16", 2, 48, 48)
    m_a, m_b = _model(scale, "bf16", 1), _model(scale, "bf16", 1)
    ts = TrainStep(m_a, world_size=1, accum_steps=2, lambda_ssim=lam["ssim"], lambda_msssim=lam["msssim"], lambda_fft=lam["fft"],
                   lambda_vif=lam["vif"], perceptual_loss=ts_tower, lambda_perceptual=LAM)
    ts.forward_backward(x[0:1], hr[0:1])
    loss = ts.forward_backward(x[1:2], hr[1:2])
    torch.cuda.synchronize()
    scratch = {n: torch.empty(getattr(lib, f"m2t_{n}_loss_scratch_bytes")(1, 3, Hs, Ws), dtype=torch.uint8, device="cuda") for n in lam}
    # the global counts of a cycle of two micro-batches of one image: map entries, (image, channel) pairs, reals of the half spectrum, images
    div = {"ssim": float(2 * 3 * (Hs - 10) * (Ws - 10)), "msssim": 6.0, "fft": float(2 * 3 * Hs * (Ws // 2 + 1) * 2), "vif": 2.0}
    parts = []
    for i in range(2):
        cx, ch = x[i:i + 1].contiguous(), hr[i:i + 1].contiguous()
        plan = m_b._plan_for(cx)
        ws, st, h = _lib.ptr(plan.workspace), _lib.stream_ptr(), _lib.ptr(ch)
        v = {n: torch.full((1,), float("nan"), device="cuda") for n in names}
        grads = torch.full_like(m_b.flat_params, float("nan"))
        _forward(lib, m_b, plan, cx)
        assert _pixel(lib, plan, ch, v["l1"], divisor=hr.numel()) == 0
        _lib.check(lib.m2t_ssim_loss(plan.handle, h, lam["ssim"], div["ssim"], 1.0, _lib.ptr(v["ssim"]), 0, _lib.ptr(scratch["ssim"]), ws, st),
                   "m2t_ssim_loss")
        _lib.check(lib.m2t_msssim_loss(plan.handle, h, lam["msssim"], div["msssim"], 1.0, _lib.ptr(v["msssim"]), 0, _lib.ptr(scratch["msssim"]),
                                       ws, st), "m2t_msssim_loss")
        _lib.check(lib.m2t_fft_loss(plan.handle, h, lam["fft"], div["fft"], 1.0, 0, _lib.ptr(v["fft"]), 0, _lib.ptr(scratch["fft"]), ws, st),
                   "m2t_fft_loss")
        _lib.check(lib.m2t_vif_loss(plan.handle, h, lam["vif"], div["vif"], 1.0, _lib.VIF_SIGMA_N_SQ, _lib.ptr(v["vif"]), 0,
                                    _lib.ptr(scratch["vif"]), ws, st), "m2t_vif_loss")
        assert _vgg(lib, plan, ts_tower, ch, v["perceptual"], divisor=2) == 0
        _backward(lib, m_b, plan, cx, grads)
        torch.cuda.synchronize()
        parts.append((v, grads))
    got = dict(zip(names, (ts.l1_loss, ts.ssim_loss, ts.msssim_loss, ts.fft_loss, ts.vif_loss, ts.perceptual_loss_value)))
    for n in names:
        want = parts[0][0][n] + parts[1][0][n]
        assert bool(torch.isfinite(want).all()) and float(want) != 0.0, n
        assert torch.equal(got[n], want), (n, float(got[n]), float(want))
    assert torch.equal(loss, got["l1"] + got["ssim"] + got["msssim"] + got["fft"] + got["vif"] + got["perceptual"])
    assert_flat_equal(m_a, ts.grads, parts[0][1] + parts[1][1], "accumulated pixel + SSIM + MS-SSIM + FFT + VIF + perceptual")
    ts.optimizer_step()
    assert ts.micro_count == 0
