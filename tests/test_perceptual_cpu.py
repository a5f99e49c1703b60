"""CPU tests (no GPU) of the VGG19 feature loss (losses.PerceptualLoss, m2t_vgg_* of include/m2t_perceptual.h): the fp64 restatement the
GPU tests compare the kernels with (tests/vgg_ref.py) -- its teacher-forced backward against torch autograd, and the gradient gate
against one-line faults -- the batch-norm fold, the name mapping, the C ABI table, and argument validation on the host."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import vgg_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD = V.random_weights(11)


def _pair(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(shape, generator=g) * (hi - lo) + lo
    x = (y + 0.1 * (hi - lo) * torch.randn(shape, generator=g)).float()
    return x, y.float()


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("crit", ["l1", "sl1", "l2"])
@pytest.mark.parametrize("shape,R,clamp", [((2, 3, 40, 48), 1.0, False), ((1, 1, 33, 47), 255.0, True)], ids=["2x3x40x48", "1x1x33x47-clamp"])
def test_teacher_forced_backward_equals_autograd_of_the_exact_forward(shape, R, clamp, crit):
    """With masks, arg-maxes and signs taken from the exact forward's own activations the teacher-forced backward IS its gradient: the
    difference to autograd is rounding, about 1e-12 of the largest entry."""
    x, y = _pair(shape, 3, -0.1 * R, 1.1 * R)
    tw = (1.0, 0.5, 0.0, 2.0, 1.5)
    leaf = x.double().clone().requires_grad_(True)
    ws, bs = V.weight_list(SD, False)
    xa = V._tower(V.normalise(leaf, R, clamp, False), ws, bs, False)
    ya = V.forward_exact(y, SD, R, False)
    yt = [ya[l] for l in V.TAP_LAYERS]
    loss, means = V.loss_from_taps([xa[l] for l in V.TAP_LAYERS], yt, tw, crit, 0.7)
    loss.backward()
    gx = V.backward([a.detach() for a in xa], yt, SD, x, crit, tw, 0.7, R, clamp, rounded=False)
    assert gx.shape == x.shape and float(leaf.grad.abs().max()) > 0
    err = float((gx - leaf.grad).abs().max() / leaf.grad.abs().max())
    print(f"{shape} {crit}: teacher-forced against autograd {err:.3e}")
    assert err <= 1e-11, err
    if clamp:
        out = (x < 0) | (x > R)
        assert int(out.sum()) > 0 and int(torch.count_nonzero(gx[out])) == 0
    # odd sizes: the row / column dropped by the floor gets no gradient through the pool
    if shape[2] % 2:
        a1 = xa[1].detach()
        g = V.pool_backward(a1, torch.ones(a1.shape[0], a1.shape[1], a1.shape[2] // 2, a1.shape[3] // 2, dtype=torch.float64))
        assert int(torch.count_nonzero(g[:, :, -1, :])) == 0 and int(torch.count_nonzero(g[:, :, :, -1])) == 0


def test_pool_backward_goes_to_the_first_maximum_as_torch_does():
    g = torch.Generator().manual_seed(2)
    a = torch.randint(0, 3, (2, 8, 5, 7), generator=g).double().requires_grad_(True)          # many ties, odd sizes
    go = torch.randn(2, 8, 2, 3, generator=g, dtype=torch.float64)
    F.max_pool2d(a, 2).backward(go)
    assert torch.equal(V.pool_backward(a.detach(), go), a.grad)
    assert not torch.equal(V.pool_backward(a.detach(), go, last=True), a.grad)


def test_emulation_is_close_in_value_and_far_in_untied_gradient():
    """What shapes the tests: the value of the bf16 emulation is within 1e-2 of fp64, so it is gated directly; the teacher-forced emulated
    backward is within 2 % of the exact one on the same masks, which is what makes MARGIN x that a usable budget."""
    x, y = _pair((1, 3, 40, 48), 5)
    ex, ey = V.forward_exact(x, SD), V.forward_exact(y, SD)
    mx, my = V.forward_emulated(x, SD), V.forward_emulated(y, SD)
    le, _ = V.loss_from_taps([ex[l] for l in V.TAP_LAYERS], [ey[l] for l in V.TAP_LAYERS], (1.0,) * 5, "l1")
    lm, _ = V.loss_from_taps([mx[l] for l in V.TAP_LAYERS], [my[l] for l in V.TAP_LAYERS], (1.0,) * 5, "l1")
    assert abs(float(lm - le)) <= 1e-2 * float(le)
    yt = [my[l] for l in V.TAP_LAYERS]
    exact = V.backward(mx, yt, SD, x, rounded=False)
    emul = V.backward(mx, yt, SD, x, rounded=True)
    ok, err, budget = V.grad_gate(emul, exact, emul)
    print(f"emulated backward on its own masks: {err:.3e} of the largest entry")
    assert ok and 1e-4 < err < 2e-2


# ------------------------------------------------------------------------------------------------------------- the gate's self-test
@pytest.fixture(scope="module")
def tied():
    """an emulated forward whose pre-pool activations are coarsely quantised, so that pool windows hold tied maxima"""
    x, y = _pair((1, 3, 40, 48), 7)
    mx, my = V.forward_emulated(x, SD), V.forward_emulated(y, SD)
    for l in (1, 3, 7, 11):
        mx[l] = torch.round(mx[l] * 2.0) / 2.0
    yt = [my[l] for l in V.TAP_LAYERS]
    exact = V.backward(mx, yt, SD, x, rounded=False)
    emul = V.backward(mx, yt, SD, x, rounded=True)
    return x, mx, yt, exact, emul


def test_gradient_gate_accepts_the_emulation_and_a_second_rounding(tied):
    x, mx, yt, exact, emul = tied
    assert V.grad_gate(emul, exact, emul)[0]
    assert V.grad_gate(exact + 2.0 * (emul - exact), exact, emul)[0]


@pytest.mark.parametrize("fault", V.FAULTS)
def test_gradient_gate_rejects_one_line_faults(tied, fault):
    x, mx, yt, exact, emul = tied
    bad = V.backward(mx, yt, SD, x, rounded=True, fault=fault)
    ok, err, budget = V.grad_gate(bad, exact, emul)
    print(f"{fault}: {err:.3e} against a budget of {budget:.3e}")
    assert not ok, (fault, err, budget)


# ------------------------------------------------------------------------------------------------------------- weights
def _bn_state(seed):
    from m2trans_amd.losses import _VGG19_BN_CONVS
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, ci, co in zip(_VGG19_BN_CONVS, V.CIN, V.COUT):
        sd[f"features.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * 0.1
        sd[f"features.{i}.bias"] = torch.randn(co, generator=g) * 0.1
        sd[f"features.{i + 1}.weight"] = torch.rand(co, generator=g) + 0.5
        sd[f"features.{i + 1}.bias"] = torch.randn(co, generator=g) * 0.1
        sd[f"features.{i + 1}.running_mean"] = torch.randn(co, generator=g) * 0.1
        sd[f"features.{i + 1}.running_var"] = torch.rand(co, generator=g) + 0.5
        sd[f"features.{i + 1}.num_batches_tracked"] = torch.tensor(3)
    sd["classifier.0.weight"] = torch.zeros(4, 4)
    return sd


def test_batch_norm_fold_equals_eval_mode_conv_and_bn_in_fp64():
    from m2trans_amd.losses import _VGG19_BN_CONVS, vgg_fold_state_dict
    sd = _bn_state(4)
    folded = vgg_fold_state_dict(sd)
    g = torch.Generator().manual_seed(9)
    for plain, bn, ci in zip(V.LAYERS, _VGG19_BN_CONVS, V.CIN):
        a = torch.randn(1, ci, 6, 5, generator=g, dtype=torch.float64)
        z = F.conv2d(a, sd[f"features.{bn}.weight"].double(), sd[f"features.{bn}.bias"].double(), padding=1)
        ref = F.batch_norm(z, sd[f"features.{bn + 1}.running_mean"].double(), sd[f"features.{bn + 1}.running_var"].double(),
                           sd[f"features.{bn + 1}.weight"].double(), sd[f"features.{bn + 1}.bias"].double(), training=False, eps=1e-5)
        got = F.conv2d(a, folded[f"features.{plain}.weight"].double(), folded[f"features.{plain}.bias"].double(), padding=1)
        assert folded[f"features.{plain}.weight"].dtype == torch.float32
        assert float((got - ref).abs().max()) <= 2e-6 * float(ref.abs().max())       # the one fp32 rounding of the folded tensors


def test_name_mapping_for_both_schemes_and_prefixes():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import vgg_fold_state_dict, vgg_param_names
    names = vgg_param_names()
    assert len(names) == 26 and names[0] == "features.0.weight" and names[-1] == "features.28.bias"
    for prefix in ("", "vgg.", "module.vgg."):
        out = vgg_fold_state_dict({prefix + k: v for k, v in SD.items()})
        assert sorted(out) == sorted(names) and all(torch.equal(out[k], SD[k]) for k in names)
    bare = vgg_fold_state_dict({k[len("features."):]: v for k, v in SD.items()})          # the Sequential's own keys
    assert all(torch.equal(bare[k], SD[k]) for k in names)
    deeper = dict(SD)
    deeper["features.30.weight"] = torch.zeros(512, 512, 3, 3)                            # conv5_2 and the classifier are ignored
    assert sorted(vgg_fold_state_dict(deeper)) == sorted(names)
    bn = vgg_fold_state_dict({"vgg.features." + k[len("features."):]: v for k, v in _bn_state(1).items() if k.startswith("features.")})
    assert sorted(bn) == sorted(names)
    with pytest.raises(M2TError, match="missing"):
        vgg_fold_state_dict({k: v for k, v in SD.items() if k != "features.19.bias"})


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_tower_constants_are_the_references():
    from m2trans_amd import _lib
    assert _lib.VGG_MIN_SIDE == 16 and _lib.VGG_LAYERS == V.LAYERS and _lib.VGG_CHANNELS == V.COUT and _lib.VGG_TAP_LAYERS == V.TAP_LAYERS


def test_tower_object_inventory_and_workspace_layout_on_the_host():
    from m2trans_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.m2t_vgg_create(C.byref(h), _lib.F32) == -2 and b"bf16 only" in lib.m2t_last_error_string()
    assert lib.m2t_vgg_create(C.byref(h), 7) == -2 and lib.m2t_vgg_create(None, _lib.BF16) == -2
    assert lib.m2t_vgg_create(C.byref(h), _lib.BF16) == 0
    try:
        total = sum(co * ci * 9 + co for ci, co in zip(V.CIN, V.COUT))
        assert lib.m2t_vgg_query(h, b"num_params") == total and lib.m2t_vgg_query(h, b"num_param_tensors") == 26
        assert lib.m2t_vgg_query(h, b"loaded") == 0 and lib.m2t_vgg_query(h, b"nonsense") == -1
        off = 0
        for k, (i, ci, co) in enumerate(zip(V.LAYERS, V.CIN, V.COUT)):
            assert lib.m2t_vgg_param_name(h, 2 * k) == f"features.{i}.weight".encode()
            assert lib.m2t_vgg_param_name(h, 2 * k + 1) == f"features.{i}.bias".encode()
            assert lib.m2t_vgg_query(h, f"param:features.{i}.weight".encode()) == off
            assert lib.m2t_vgg_query(h, f"numel:features.{i}.weight".encode()) == co * ci * 9
            off += co * ci * 9
            assert lib.m2t_vgg_query(h, f"param:features.{i}.bias".encode()) == off
            off += co
        assert lib.m2t_vgg_param_name(h, 26) is None
        # two packings (forward; flipped and transposed) of every MFMA layer in bf16
        assert lib.m2t_vgg_query(h, b"packed_bytes") >= 2 * 2 * (total - 64 * 27 - sum(V.COUT))
        one = C.c_void_p(8)
        tw = (C.c_double * 5)(1, 1, 1, 1, 1)
        call = lambda **kw: lib.m2t_vgg_loss_tensor(*[kw.get(k, v) for k, v in (
            ("v", h), ("x", one), ("y", one), ("B", 1), ("C", 3), ("H", 16), ("W", 24), ("xs", 3 * 16 * 24), ("rs", 24), ("dr", 1.0), ("clamp", 1),
            ("kind", 0), ("param", 0.0), ("tw", tw), ("scale", 1.0), ("gx", None), ("loss", one), ("per", None), ("acc", 0), ("ws", one),
            ("stream", None))])
        nan = (C.c_double * 5)(1, 1, float("nan"), 1, 1)
        for bad in (dict(v=None), dict(x=None), dict(y=None), dict(loss=None), dict(ws=None), dict(H=15), dict(W=15), dict(B=0), dict(B=32768),
                    dict(C=2, xs=2 * 16 * 24), dict(dr=0.0), dict(dr=float("nan")), dict(kind=4), dict(kind=-1), dict(kind=3, param=0.0),
                    dict(tw=None), dict(tw=nan), dict(scale=float("inf")), dict(rs=23), dict(xs=3 * 16 * 24 + 1)):
            assert call(**bad) == -2, bad
        assert call(H=15) == -2 and b"at least 16" in lib.m2t_last_error_string()
        assert call() == -3 and b"m2t_vgg_load_weights first" in lib.m2t_last_error_string()      # every argument fine, no weights: a state error
        assert lib.m2t_vgg_conv_forward(h, 1, one, one, 1, 8, 8, 1.0, None) == -3
        assert lib.m2t_vgg_conv_forward(h, 13, one, one, 1, 8, 8, 1.0, None) == -2
        assert lib.m2t_vgg_conv_backward(h, 1, one, None, None, 1, 8, 8, 1.0, None) == -2
        assert lib.m2t_vgg_pool_forward(one, one, 1, 5, 7, 12, None) == -2 and lib.m2t_vgg_pool_forward(one, one, 1, 1, 7, 8, None) == -2
        assert lib.m2t_vgg_pool_backward(one, None, one, 1, 5, 7, 8, 0, None) == -2
        assert lib.m2t_vgg_loss(None, h, one, 1.0, 1.0, 1.0, 0, 0.0, tw, one, 0, one, one, None) == -2
    finally:
        lib.m2t_vgg_destroy(h)
    bad_off = C.c_size_t(-1).value
    assert lib.m2t_vgg_workspace_bytes(1, 15, 64, 1) == 0 and lib.m2t_vgg_workspace_bytes(1, 64, 15, 0) == 0 and lib.m2t_vgg_workspace_bytes(0, 64, 64, 0) == 0
    v, g = lib.m2t_vgg_workspace_bytes(2, 40, 48, 0), lib.m2t_vgg_workspace_bytes(2, 40, 48, 1)
    acts = sum(2 * 2 * (40 >> lv) * (48 >> lv) * co for lv, co in zip(V.LEVEL, V.COUT))
    assert v > acts and g >= v + acts
    offs = [lib.m2t_vgg_workspace_offset(2, 40, 48, 0, l) for l in range(13)] + [lib.m2t_vgg_workspace_offset(2, 40, 48, 1, k) for k in range(5)] \
        + [lib.m2t_vgg_workspace_offset(2, 40, 48, 2, k) for k in range(5)]
    assert offs == sorted(offs) and len(set(offs)) == len(offs) and offs[0] == 0 and all(o % 256 == 0 for o in offs) and offs[-1] < v
    goffs = [lib.m2t_vgg_workspace_offset(2, 40, 48, 3, l) for l in range(13)]
    assert goffs == sorted(goffs) and v <= goffs[0] and goffs[-1] + 2 * 2 * 2 * 3 * 512 <= g
    for bad in ((2, 40, 48, 0, 13), (2, 40, 48, 1, 5), (2, 40, 48, 2, -1), (2, 40, 48, 4, 0), (2, 15, 48, 0, 0)):
        assert lib.m2t_vgg_workspace_offset(*bad) == bad_off, bad


def test_python_entry_validates_arguments_without_a_gpu():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import PerceptualLoss
    with pytest.raises(NotImplementedError, match="not implemented"):
        PerceptualLoss(criterion="huber")
    for kw in (dict(weights=[1.0] * 4), dict(weights=[1.0, 1.0, float("nan"), 1.0, 1.0]), dict(data_range=0.0), dict(data_range=float("inf"))):
        with pytest.raises(M2TError):
            PerceptualLoss(**kw)
    p = PerceptualLoss(device="cpu")
    assert p.weights == [1.0] * 5 and p.resize is False and p.criterion == "l1" and not p.loaded
    assert (PerceptualLoss(criterion="sl1", device="cpu").kind, PerceptualLoss(criterion="l2", device="cpu").kind) == (3, 1)
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(M2TError, match="no VGG19 weights loaded"):
        p(x, x)
    with pytest.raises(M2TError, match="at least 16"):
        p(x[..., :15], x[..., :15])
    with pytest.raises(M2TError, match="1 or 3 channels"):
        p(x[:, :2], x[:, :2])
    with pytest.raises(M2TError, match="equal shape"):
        p(x, x[..., :20])
    with pytest.raises(M2TError, match="HIP device"):
        p.load_vgg_state_dict(SD)                                       # a host "device": no fallback
    with pytest.raises(M2TError, match="missing"):
        p.load_vgg_state_dict({})


# ------------------------------------------------------------------------------------------------------------- TrainStep
class _Calls:
    """A stand-in for the loaded library: records the entry points in call order, every call succeeds."""

    def __init__(self):
        self.names, self.args = [], {}

    def __getattr__(self, name):
        def fn(*a):
            self.names.append(name)
            self.args[name] = a
            return 1 << 20 if name.endswith("_bytes") else 0
        return fn


def _fake_tower(**kw):
    import types
    d = dict(loaded=True, resize=False, data_range=1.0, criterion="sl1", weights=[1.0, 0.5, 0.0, 2.0, 1.5], kind=3, param=1.0, handle="H",
             tap_weights=lambda: "TW", workspace=lambda B, H, W, g: ("WS", B, H, W, g))
    d.update(kw)
    return types.SimpleNamespace(**d)


def _host_step(monkeypatch, perceptual=None, **terms):
    """TrainStep.forward_backward on the host against _Calls: the step object assembled without __init__, no device needed."""
    import contextlib
    import types
    from m2trans_amd import _lib, train_step as T
    calls = _Calls()
    monkeypatch.setattr(_lib, "load", lambda: calls)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(_lib, "ptr", lambda t: t if isinstance(t, tuple) else None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    plan = types.SimpleNamespace(handle=None, workspace=None, gen=0, trained=False)
    model = types.SimpleNamespace(scale=2, rgb_range=1.0, flat_params=torch.zeros(4), _plan_for=lambda lr: plan)
    ts = T.TrainStep.__new__(T.TrainStep)
    ts.model, ts.micro_count, ts.accum_steps, ts.world_size = model, 0, 1, 1
    ts.semantic_loss, ts.lambda_clip, ts.lambda_l1 = None, 0.0, 1.0
    ts.grads, ts.micro_grads, ts.l1_loss, ts.micro_loss = torch.zeros(4), None, torch.zeros(1), None
    ts.set_pixel_loss("l1", None)
    ts.ssim_loss = ts.msssim_loss = ts.fft_loss = ts.vif_loss = None
    ts._ssim_scratch, ts._msssim_scratch, ts._fft_scratch, ts._vif_scratch, ts.fft_norm = {}, {}, {}, {}, "backward"
    ts.lambda_ssim, ts.lambda_msssim, ts.lambda_fft, ts.lambda_vif = 0.0, 0.0, 0.0, 0.0
    for k, v in terms.items():
        if k != "lambda_perceptual":
            setattr(ts, k, v)
            setattr(ts, k.replace("lambda_", "") + "_loss", torch.zeros(1))
    if "lambda_perceptual" in terms:
        ts.perceptual_loss = perceptual
        ts.set_lambda_perceptual(terms["lambda_perceptual"])
    ts.forward_backward(torch.zeros(2, 3, 24, 24), torch.zeros(2, 3, 48, 48))
    return ts, calls


def test_lambda_perceptual_resolver_default_and_requirements():
    import inspect
    import types
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep, perceptual_size_supported, resolve_lambda_perceptual
    sig = inspect.signature(TrainStep.__init__).parameters
    assert sig["lambda_perceptual"].default == 0.0 and sig["perceptual_loss"].default is None
    assert resolve_lambda_perceptual(0) == 0.0 and resolve_lambda_perceptual("0.5") == 0.5
    for bad in (-0.1, float("nan"), float("inf"), None, "much"):
        with pytest.raises(M2TError):
            resolve_lambda_perceptual(bad)
    assert perceptual_size_supported(16, 16) and not perceptual_size_supported(15, 400) and not perceptual_size_supported(400, 15)
    ts = TrainStep.__new__(TrainStep)
    ts.model = types.SimpleNamespace(rgb_range=1.0, flat_params=torch.zeros(1))
    ts.accum_steps, ts.micro_count = 2, 1
    with pytest.raises(M2TError, match="accumulation cycle"):
        ts.set_lambda_perceptual(0.0)
    ts.micro_count = 0
    ts.set_lambda_perceptual(0.0)
    assert ts.lambda_perceptual == 0.0 and ts.perceptual_loss_value is None
    for tower, what in ((None, "needs perceptual_loss="), (_fake_tower(loaded=False), "no VGG19 weights loaded"),
                        (_fake_tower(resize=True), "resize=True"), (_fake_tower(data_range=255.0), "rgb_range")):
        ts.perceptual_loss = tower
        with pytest.raises(M2TError, match=what):
            ts.set_lambda_perceptual(0.1)
    ts.perceptual_loss = _fake_tower()
    ts.set_lambda_perceptual(0.1)
    assert ts.lambda_perceptual == 0.1 and ts.perceptual_loss_value.shape == (1,)
    with pytest.raises(M2TError, match="at least 16"):
        ts._perceptual_workspace_for(torch.zeros(2, 3, 12, 64))


def test_lambda_perceptual_zero_issues_todays_calls_and_the_term_runs_last_before_the_backward(monkeypatch):
    today = ["m2t_forward", "m2t_l1_loss_deferred", "m2t_backward"]
    _, bare = _host_step(monkeypatch)                                    # a step object that knows nothing of the term
    ts, zero = _host_step(monkeypatch, perceptual=_fake_tower(), lambda_perceptual=0.0)
    assert bare.names == today and zero.names == today and ts.perceptual_loss_value is None
    ts, on = _host_step(monkeypatch, perceptual=_fake_tower(), lambda_perceptual=0.05)
    assert on.names == ["m2t_forward", "m2t_l1_loss", "m2t_vgg_loss", "m2t_backward"]
    a = on.args["m2t_vgg_loss"]
    # tower, weight, divisor = B, R, kind, param, tap weights, store (first micro-batch), the tower's workspace with the gradient regions
    assert a[1] == "H" and a[3] == 0.05 and a[4] == 2.0 and a[5] == 1.0 and a[6:9] == (3, 1.0, "TW") and a[10] == 0 and a[11] == ("WS", 2, 48, 48, True)
    _, every = _host_step(monkeypatch, perceptual=_fake_tower(), lambda_ssim=0.1, lambda_fft=0.1, lambda_vif=0.05, lambda_perceptual=0.05)
    order = [n for n in every.names if not n.endswith("_bytes")]
    assert order == ["m2t_forward", "m2t_l1_loss", "m2t_ssim_loss", "m2t_fft_loss", "m2t_vif_loss", "m2t_vgg_loss", "m2t_backward"]


class _Step:
    """The flat-buffer part of TrainStep on the CPU with the perceptual term's settings."""

    def __init__(self, m, tower=None, lambda_perceptual=0.0, step_count=7):
        from m2trans_amd.train_step import TrainStep
        g = torch.Generator().manual_seed(step_count)
        self.exp_avg = torch.randn(m.flat_params.shape, generator=g)
        self.exp_avg_sq = torch.rand(m.flat_params.shape, generator=g)
        self.step_count, self.lr, self.scheduler_last_epoch, self.micro_count, self.accum_steps = step_count, 5e-5, 0, 0, 1
        TrainStep.set_pixel_loss(self, "l1", None)
        self.perceptual_loss, self.lambda_perceptual = tower, lambda_perceptual

    def set_pixel_loss(self, name, param=None):
        from m2trans_amd.train_step import TrainStep
        TrainStep.set_pixel_loss(self, name, param)

    def set_lambda_perceptual(self, value):
        self.lambda_perceptual = float(value)

    def set_lr(self, lr):
        self.lr = lr


def test_checkpoint_carries_the_settings_when_the_term_is_on_and_nothing_when_it_is_off():
    import types
    from m2trans_amd._lib import M2TError
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    from m2trans_amd.losses import PerceptualLoss
    from m2trans_amd.M2Trans_network import create_model
    model = lambda: create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))
    m = model()
    keys = ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict"]
    off = export_checkpoint(m, _Step(m, PerceptualLoss(device="cpu"), 0.0), epoch=3)
    assert list(off) == keys                                             # the key is absent: today's dict
    src = _Step(m, PerceptualLoss(weights=[1.0, 0.5, 0.0, 2.0, 1.5], criterion="sl1", device="cpu"), 0.05)
    ck = export_checkpoint(m, src, epoch=3)
    assert list(ck) == keys + ["m2t_loss"]
    assert ck["m2t_loss"] == {"pixel_loss": "l1", "param": None, "lambda_perceptual": 0.05, "perceptual_criterion": "sl1",
                              "perceptual_weights": [1.0, 0.5, 0.0, 2.0, 1.5], "perceptual_resize": False}
    flat = [k for k in ck["m2t_loss"]] + [k for k in ck["model_state_dict"]]
    assert not any("features." in k or "vgg" in k for k in flat)        # never the VGG19 weights
    dst = _Step(model(), PerceptualLoss(device="cpu"), 0.0, step_count=1)
    assert import_checkpoint(ck, model(), dst) == 4
    p = dst.perceptual_loss
    assert dst.lambda_perceptual == 0.05 and (p.criterion, p.kind, p.param, p.weights, p.resize) == ("sl1", 3, 1.0, [1.0, 0.5, 0.0, 2.0, 1.5], False)
    with pytest.raises(M2TError, match="perceptual_loss="):
        import_checkpoint(ck, model(), _Step(model(), None, 0.0))
