"""-m gpu: the pixel-loss family of TrainStep (l1, mse, charbonnier, smooth_l1; m2t_pixel_loss / m2t_pixel_loss_deferred) -- the
per-pixel function against fp64 (tests/pixel_loss_ref.py), the seed taken inside the fused x4 tail backward against the stand-alone
kernel, the deferred request against the immediate one on every unfused route, TrainStep against the autograd route through torch's
own loss modules, and the L1 path against the entry points it had before the family existed.

Inputs: the closed-form parameters give a pre-clamp output within a few hundredths of 0, which never meets the upper clamp.  The last
tail conv (no bias) is therefore scaled, which scales the pre-clamp output exactly; every test that relies on coverage reads it back
and requires that each class a kind treats differently -- below 0, above R, inside with |d| below / not below beta, d > 0, d < 0 --
holds at least 5 % of the pixels."""
import ctypes as C

import pytest
import torch

from oracle import m2trans_oracle as O
from tests import pixel_loss_ref as R
from tests.gpu_util import assert_flat_equal, build_model

pytestmark = pytest.mark.gpu

NB = 2
BETA = 0.25
KINDS = [("l1", None), ("mse", None), ("charbonnier", 1e-6), ("smooth_l1", BETA)]
KIND_IDS = [k for k, _ in KINDS]
SHAPES = [(2, 40, 56), (2, 64, 96)]          # reflect-padded (the crop matters); border and interior tiles
TAIL_GAIN = {4: ("tail.6.weight", 100.0), 3: ("tail.3.weight", 5.0), 2: ("tail.3.weight", 28.0)}
_PARAMS = {}


def _params(scale, nb=NB):
    if (scale, nb) not in _PARAMS:
        p = {k: v.clone() for k, v in O.closed_form_params(64, scale, nb).items()}
        name, gain = TAIL_GAIN[scale]
        p[name] = p[name] * gain
        _PARAMS[(scale, nb)] = p
    return _PARAMS[(scale, nb)]


def _model(scale, dtype, nb=NB):
    return build_model(scale, nb, dtype, params=_params(scale, nb))[0]


def _images(B, H, W, scale, step=0):
    x = O.closed_form_image(B, 3, H, W, phase=0.37 * step).cuda()
    hr = O.closed_form_image(B, 3, H * scale, W * scale, phase=0.7 + 0.91 * step).cuda()
    return x, hr


def _srpre(plan, B, scale):
    Hp, Wp = plan.query("padded_h") * scale, plan.query("padded_w") * scale
    return plan.ws_tensor("srpre", dtype=torch.float32).view(B, 3, Hp, Wp)


def _require_coverage(pre, hr, tag):
    """pre: the pre-clamp output read back (padded size), hr the target.  A condition on the inputs, not a tolerance."""
    Hs, Ws = hr.shape[-2:]
    v = pre[..., :Hs, :Ws].double().cpu()
    d = v.clamp(0, 1) - hr.double().cpu()
    inside = (v >= 0) & (v <= 1)
    share = {"below 0": v < 0, "above 1": v > 1, "inside, |d| < beta": inside & (d.abs() < BETA),
             "inside, |d| >= beta": inside & (d.abs() >= BETA), "inside, d > 0": inside & (d > 0), "inside, d < 0": inside & (d < 0)}
    share = {k: float(m.double().mean()) for k, m in share.items()}
    assert min(share.values()) >= 0.05, f"{tag}: the inputs do not cover every class: {share}"


def _kind_args(kind, param):
    return R.KINDS[kind], float(param or 0.0)


def _forward(lib, model, plan, x):
    from m2trans_amd import _lib
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(x), None, 1.0, 1, _lib.ptr(plan.workspace),
                               _lib.stream_ptr()), "m2t_forward")


def _pixel_loss(lib, plan, kind, param, hr, out, deferred=False, divisor=None):
    from m2trans_amd import _lib
    k, p = _kind_args(kind, param)
    fn = lib.m2t_pixel_loss_deferred if deferred else lib.m2t_pixel_loss
    _lib.check(fn(plan.handle, k, p, _lib.ptr(hr), 1.0, float(hr.numel() if divisor is None else divisor), 1.0, _lib.ptr(out),
                  _lib.ptr(plan.workspace), _lib.stream_ptr()), "m2t_pixel_loss" + ("_deferred" if deferred else ""))


def _backward(lib, model, plan, x, grads):
    from m2trans_amd import _lib
    _lib.check(lib.m2t_backward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(x), _lib.ptr(grads), _lib.ptr(plan.workspace),
                                _lib.stream_ptr()), "m2t_backward")


def _by_hand(model, plan, x, hr, kind, param, deferred=False, divisor=None):
    """(loss [1], gradients): m2t_forward -> m2t_pixel_loss(_deferred) -> m2t_backward into fresh buffers."""
    from m2trans_amd import _lib
    lib = _lib.load()
    loss = torch.full((1,), float("nan"), device="cuda")
    grads = torch.full_like(model.flat_params, float("nan"))
    _forward(lib, model, plan, x)
    _pixel_loss(lib, plan, kind, param, hr, loss, deferred, divisor)
    _backward(lib, model, plan, x, grads)
    torch.cuda.synchronize()
    return loss, grads


def _options(plan, opts):
    from m2trans_amd import _lib
    for key, val in opts.items():
        _lib.check(_lib.load().m2t_set_option(plan.handle, key.encode(), val), "m2t_set_option " + key)


# ------------------------------------------------------------------ 1. seed and value, per pixel, against fp64
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("scale,shape", [(2, SHAPES[0]), (3, SHAPES[0]), (4, SHAPES[0]), (4, SHAPES[1])])
def test_seed_and_value_of_every_kind_against_fp64(dtype, scale, shape):
    """The immediate m2t_pixel_loss on the forward's own pre-clamp output (read back: the reference sees the bits the kernel saw).
    Seed: |got - ref| <= 1e-6 |ref| + 1e-7 sc per pixel -- the function is at most six fp32 roundings (3.6e-7), 1e-6 leaves room for
    a 1-ulp reciprocal root and rejects any wrong branch or factor; exactly 0 outside the crop and where the clamp is active.  Value:
    1e-5 relative to the fp64 sum (a thread adds a few tens of same-sign terms before the fixed-order tree: 2e-6 at worst; a missing
    0.5, 2 or 1 / beta is off by far more)."""
    from m2trans_amd import _lib
    lib = _lib.load()
    B, H, W = shape
    model = _model(scale, dtype)
    x, hr = _images(B, H, W, scale)
    plan = model._plan_for(x)
    _forward(lib, model, plan, x)
    torch.cuda.synchronize()
    pre = _srpre(plan, B, scale).clone()
    _require_coverage(pre, hr, f"{dtype} x{scale} {shape}")
    Hs, Ws = hr.shape[-2:]
    assert tuple(pre.shape[-2:]) != (Hs, Ws) or shape != SHAPES[0], "(2, 40, 56) is meant to be reflect-padded"
    sc = float(torch.tensor(1.0 / hr.numel(), dtype=torch.float32))
    out = torch.full((1,), float("nan"), device="cuda")
    pad = torch.ones(pre.shape, dtype=torch.bool)
    pad[..., :Hs, :Ws] = False
    clamped = ((pre < 0) | (pre > 1)).cpu()
    for kind, param in KINDS:
        plan.ws_tensor("gpre", dtype=torch.float32).fill_(float("nan"))
        _pixel_loss(lib, plan, kind, param, hr, out)
        torch.cuda.synchronize()
        got = plan.ws_tensor("gpre", dtype=torch.float32).view(pre.shape).double().cpu()
        want_loss, want = R.loss_and_seed(kind, pre.cpu(), hr.cpu(), param)
        tag = f"{kind} {dtype} x{scale} {shape}"
        assert bool(torch.isfinite(got).all()), tag
        assert int(torch.count_nonzero(got[pad])) == 0, f"{tag}: seed outside the crop"
        assert int(torch.count_nonzero(got[clamped])) == 0, f"{tag}: seed where the clamp is active"
        assert int(torch.count_nonzero(want)) > 0.2 * hr.numel()
        excess = (got - want).abs() - (1e-6 * want.abs() + 1e-7 * sc)
        assert float(excess.max()) <= 0.0, f"{tag}: seed off by {float(excess.max()):.3e} beyond the gate ({int((excess > 0).sum())} pixels)"
        assert abs(float(out) - float(want_loss)) <= 1e-5 * abs(float(want_loss)), (tag, float(out), float(want_loss))


# ------------------------------------------------------------------ 2. fused = stand-alone, bit for bit
@pytest.mark.parametrize("mfma32", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind,param", KINDS, ids=KIND_IDS)
def test_seed_inside_the_fused_tail_backward_is_bit_identical_for_every_kind(kind, param, shape, mfma32):
    """bf16 x4: TrainStep(pixel_loss=kind) with "fused_l1" 1 (the seed taken by the recomputing tail backward, either kernel) against 0
    (m2t_backward runs the clamp kernel first) and the immediate m2t_pixel_loss as a third arm.  One per-pixel function -> every gradient
    bit-identical; the fused loss is the same sum in another fp32 order (2e-6, the figure of the L1 test)."""
    from m2trans_amd.train_step import TrainStep
    B, H, W = shape
    x, hr = _images(B, H, W, 4)
    res = []
    for val in (1, 0):
        model = _model(4, "bf16")
        plan = model._plan_for(x)
        _options(plan, {"tail_bwd_mfma32": mfma32, "fused_l1": val})
        assert plan.query("opt:fused_l1") == val and plan.query("opt:tail_bwd_mfma32") == mfma32
        ts = TrainStep(model, lr=1e-4, world_size=1, pixel_loss=kind, pixel_loss_param=param)
        loss = ts.forward_backward(x, hr)
        torch.cuda.synchronize()
        if val == 1:
            _require_coverage(_srpre(plan, B, 4), hr, f"{kind} {shape}")
        res.append((float(loss), ts.grads.clone()))
    model = _model(4, "bf16")
    plan = model._plan_for(x)
    _options(plan, {"tail_bwd_mfma32": mfma32})
    loss3, grads3 = _by_hand(model, plan, x, hr, kind, param)
    (l1, g1), (l0, g0) = res
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    assert_flat_equal(model, g1, g0, f"{kind}: fused against fused_l1 = 0")
    assert_flat_equal(model, g1, grads3, f"{kind}: fused against the immediate entry")
    assert l0 == float(loss3), (l0, float(loss3))
    assert abs(l1 - l0) <= 2e-6 * abs(l0), (l1, l0)


# ------------------------------------------------------------------ 3. deferred = immediate on the unfused routes
@pytest.mark.parametrize("dtype,scale,opts", [("fp32", 4, {}), ("fp32", 3, {}), ("bf16", 4, {"fused_tail": 0}), ("bf16", 2, {})],
                         ids=["fp32-x4", "fp32-x3", "bf16-x4-unfused-tail", "bf16-x2"])
@pytest.mark.parametrize("kind,param", KINDS, ids=KIND_IDS)
def test_deferred_request_equals_the_immediate_one_on_every_unfused_route(kind, param, dtype, scale, opts):
    """Where the clamp kernel runs inside m2t_backward in front of the first fork: three consecutive steps with DIFFERENT batches
    through TrainStep (deferred) against the immediate m2t_pixel_loss on a twin -- loss and every gradient bit-identical at every
    step (a stale or mis-ordered seed would carry the previous batch's values)."""
    from m2trans_amd.train_step import TrainStep
    B, H, W = SHAPES[1]

    def make():
        model = _model(scale, dtype)
        plan = model._plan_for(torch.empty(B, 3, H, W, device="cuda"))
        _options(plan, opts)
        return model, plan
    m_def, plan_d = make()
    m_imm, plan = make()
    assert plan_d.query("opt:fused_l1") == 0, "this route is meant to take the loss in front of the tail"
    ts = TrainStep(m_def, lr=1e-4, world_size=1, pixel_loss=kind, pixel_loss_param=param)
    for step in range(3):
        x, hr = _images(B, H, W, scale, step)
        loss_d = ts.forward_backward(x, hr)
        loss_i, grads_i = _by_hand(m_imm, plan, x, hr, kind, param)
        assert bool(torch.isfinite(grads_i).all()) and float(loss_i) > 0
        assert float(loss_d) == float(loss_i), (step, float(loss_d), float(loss_i))
        assert_flat_equal(m_def, ts.grads, grads_i, f"{kind} step {step}")


# ------------------------------------------------------------------ 4. against the autograd route
def _torch_loss(kind, param):
    if kind == "l1":
        return torch.nn.L1Loss()
    if kind == "mse":
        return torch.nn.MSELoss()
    if kind == "smooth_l1":
        return torch.nn.SmoothL1Loss(beta=param)
    return lambda a, b: torch.mean(torch.sqrt((a - b) * (a - b) + param))      # L1_Charbonnier_loss (reference losses.py:287-297)


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-5), ("bf16", 1e-2)])
@pytest.mark.parametrize("kind,param", KINDS, ids=KIND_IDS)
def test_train_step_matches_the_autograd_route_through_torchs_loss(kind, param, dtype, tol):
    """TrainStep(pixel_loss=kind) against loss_fn(model(x), hr).backward() on the same HIP model (the route a user had to take for
    these losses: torch's loss on the materialised output, m2t_set_output_grad).  rel-L2 of the gradients 1e-5 in fp32, 1e-2 in bf16
    (the figures of test_train_step_with_differentiable_semantic_loss); the loss value within 1e-5 in fp32."""
    from m2trans_amd.train_step import TrainStep
    B, H, W = SHAPES[0]
    model = _model(4, dtype)
    x, hr = _images(B, H, W, 4)
    ts = TrainStep(model, world_size=1, pixel_loss=kind, pixel_loss_param=param)
    loss = ts.forward_backward(x, hr)
    torch.cuda.synchronize()
    _require_coverage(_srpre(model._plan_for(x), B, 4), hr, f"{kind} {dtype}")
    got_all = ts.grads.clone()
    for prm in model.parameters():
        prm.grad = None
    want_loss = _torch_loss(kind, param)(model(x), hr)
    want_loss.backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    got, want = [], []
    for n, (o, k) in model.param_offsets().items():
        if named[n].grad is None:
            continue
        want.append(named[n].grad.reshape(-1).double().cpu())
        got.append(got_all[o:o + k].double().cpu())
    got, want = torch.cat(got), torch.cat(want)
    assert float(want.norm()) > 0
    err = float((got - want).norm() / want.norm())
    assert err <= tol, (kind, dtype, err)
    if dtype == "fp32":
        assert abs(float(loss) - float(want_loss)) <= 1e-5 * abs(float(want_loss)), (float(loss), float(want_loss))


# ------------------------------------------------------------------ 5. L1 is untouched
@pytest.mark.parametrize("dtype,fused", [("bf16", 1), ("fp32", 0)], ids=["fused", "unfused"])
def test_l1_kind_is_the_l1_entry_points_bit_for_bit(dtype, fused):
    """TrainStep(pixel_loss="l1") and the kind-0 requests against TrainStep() / m2t_l1_loss / m2t_l1_loss_deferred: loss and every
    gradient, on the route that takes the seed inside the tail backward and on one that does not."""
    from m2trans_amd import _lib
    from m2trans_amd.train_step import TrainStep
    lib = _lib.load()
    B, H, W = SHAPES[0]
    x, hr = _images(B, H, W, 4)
    out = {}
    for arm in ("default", "named"):
        model = _model(4, dtype)
        assert model._plan_for(x).query("opt:fused_l1") == fused
        ts = TrainStep(model, world_size=1) if arm == "default" else TrainStep(model, world_size=1, pixel_loss="l1")
        loss = ts.forward_backward(x, hr)
        torch.cuda.synchronize()
        out[arm] = (loss.clone(), ts.grads.clone())
    _require_coverage(_srpre(model._plan_for(x), B, 4), hr, dtype)
    for arm, deferred in (("pixel-deferred", True), ("pixel-immediate", False)):
        model = _model(4, dtype)
        out[arm] = _by_hand(model, model._plan_for(x), x, hr, "l1", None, deferred)
    for arm, fn in (("l1-deferred", lib.m2t_l1_loss_deferred), ("l1-immediate", lib.m2t_l1_loss)):
        model = _model(4, dtype)
        plan = model._plan_for(x)
        loss = torch.full((1,), float("nan"), device="cuda")
        grads = torch.full_like(model.flat_params, float("nan"))
        _forward(lib, model, plan, x)
        _lib.check(fn(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(loss), _lib.ptr(plan.workspace), _lib.stream_ptr()), arm)
        _backward(lib, model, plan, x, grads)
        torch.cuda.synchronize()
        out[arm] = (loss, grads)
    assert bool(torch.isfinite(out["default"][1]).all())
    for a, b in (("default", "named"), ("default", "pixel-deferred"), ("default", "l1-deferred"), ("l1-immediate", "pixel-immediate")):
        assert torch.equal(out[a][0], out[b][0]), (a, b, float(out[a][0]), float(out[b][0]))
        assert_flat_equal(model, out[a][1], out[b][1], f"{a} against {b}")
    # (the immediate and the deferred request differ only where the seed is fused: then by the order of the loss sum alone)
    assert_flat_equal(model, out["default"][1], out["l1-immediate"][1], "deferred against immediate")


# ------------------------------------------------------------------ 6. accumulation
def test_accumulated_charbonnier_equals_the_chunk_gradients_summed_by_torch():
    """TrainStep(accum_steps=2, pixel_loss="charbonnier") on 2 x 2 samples against the two chunks run by hand (the whole batch's
    divisor) and added with torch: gradients and loss bit for bit -- the contract of tests/test_gpu_accum.py."""
    from m2trans_amd.train_step import TrainStep
    _, H, W = SHAPES[0]
    x, hr = _images(4, H, W, 4)
    m_a, m_b = _model(4, "bf16"), _model(4, "bf16")
    ts = TrainStep(m_a, world_size=1, accum_steps=2, pixel_loss="charbonnier")
    for i in range(2):
        loss = ts.forward_backward(x[2 * i:2 * i + 2], hr[2 * i:2 * i + 2])
    torch.cuda.synchronize()
    loss = loss.clone()
    parts = []
    for i in range(2):
        cx, chr_ = x[2 * i:2 * i + 2].contiguous(), hr[2 * i:2 * i + 2].contiguous()
        parts.append(_by_hand(m_b, m_b._plan_for(cx), cx, chr_, "charbonnier", 1e-6, deferred=True, divisor=hr.numel()))
    assert torch.equal(loss, parts[0][0] + parts[1][0]), (float(loss), float(parts[0][0] + parts[1][0]))
    assert_flat_equal(m_a, ts.grads, parts[0][1] + parts[1][1], "accumulated charbonnier")
    assert float(parts[1][1].abs().max()) > 0


# ------------------------------------------------------------------ 7. the semantic-gradient route
def test_semantic_grad_route_passes_the_kind_to_the_immediate_entry():
    """TrainStep(pixel_loss="mse") with a differentiable SemanticLoss against the sequence composed by hand: m2t_forward -> the
    encoder's value and gradient -> m2t_pixel_loss -> m2t_add_output_grad -> m2t_backward.  Bit-identical."""
    from m2trans_amd import _lib
    from m2trans_amd.losses import SemanticLoss
    from m2trans_amd.train_step import TrainStep
    from oracle import swin_oracle as S
    lib = _lib.load()
    scale, nb, B, H, W = 4, 1, 2, 64, 64                         # (the shape of tests/test_gpu_semantic_grad.py's _model_and_inputs)
    x, hr = _images(B, H, W, scale)
    sl = SemanticLoss(criterion="l1", N_patches=3, device="cuda", compute_dtype="bf16", max_batch=4, differentiable=True)
    sl.load_image_encoder(S.closed_form_swin_params())
    g = torch.Generator().manual_seed(8)
    sl.set_text_features({"a": torch.randn(512, generator=g), "b": torch.randn(512, generator=g)})
    caps = ["a", "b"]
    m_a, m_b = _model(scale, "bf16", nb), _model(scale, "bf16", nb)
    ts = TrainStep(m_a, world_size=1, semantic_loss=sl, lambda_clip=0.01, pixel_loss="mse")
    torch.manual_seed(1)
    ts.forward_backward(x, hr, caps)
    torch.cuda.synchronize()
    pix_a, g_a = ts.l1_loss.clone(), ts.grads.clone()
    # by hand
    plan = m_b._plan_for(x)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    sr = torch.empty_like(hr)
    pix_b = torch.full((1,), float("nan"), device="cuda")
    g_b = torch.full_like(m_b.flat_params, float("nan"))
    torch.manual_seed(1)
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(m_b.flat_params), _lib.ptr(x), _lib.ptr(sr), 1.0, 1, ws, st), "m2t_forward")
    _, gsem, origins = sl._value_and_grad(sr, hr, caps)
    _pixel_loss(lib, plan, "mse", None, hr, pix_b)
    gsem = gsem.contiguous()
    arr = None if origins is None else (C.c_int * (2 * len(origins)))(*[int(v) for o in origins for v in o])
    _lib.check(lib.m2t_add_output_grad(plan.handle, _lib.ptr(gsem), gsem.shape[2], gsem.shape[3], arr, 0.01, 1.0, ws, st), "m2t_add_output_grad")
    _backward(lib, m_b, plan, x, g_b)
    torch.cuda.synchronize()
    assert torch.equal(pix_a, pix_b), (float(pix_a), float(pix_b))
    assert_flat_equal(m_a, g_a, g_b, "semantic-gradient route with mse")
    # the kind is live: the L1 seed gives other gradients
    _, g_l1 = _by_hand(m_b, plan, x, hr, "l1", None)
    assert not torch.equal(g_l1, g_b)


# ------------------------------------------------------------------ 8. errors
def test_pixel_loss_argument_and_state_errors():
    from m2trans_amd import _lib
    lib = _lib.load()
    ARG, STATE = -2, -3
    B, H, W = 1, 32, 32
    model = _model(4, "fp32", 1)
    x, hr = _images(B, H, W, 4)
    plan = model._plan_for(x)
    out = torch.zeros(1, device="cuda")
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()

    def call(fn, kind, param):
        return fn(plan.handle, kind, param, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(out), ws, st)
    for fn in (lib.m2t_pixel_loss, lib.m2t_pixel_loss_deferred):
        # before a forward
        for kind, param in ((0, 0.0), (1, 0.0), (2, 1e-6), (3, 1.0)):
            assert call(fn, kind, param) == STATE
    _forward(lib, model, plan, x)
    for fn in (lib.m2t_pixel_loss, lib.m2t_pixel_loss_deferred):
        for kind, param in ((4, 0.0), (-1, 0.0), (2, 0.0), (2, -1e-6), (2, float("nan")), (2, float("inf")), (3, 0.0), (3, -1.0),
                            (3, float("nan"))):
            assert call(fn, kind, param) == ARG, (kind, param)
    assert call(lib.m2t_pixel_loss, 3, 0.0) == ARG
    assert b"l1" in lib.m2t_last_error_string().replace(b"smooth_l1", b""), "beta = 0: the message names the l1 loss"
    # a refused request leaves no seed behind
    grads = torch.zeros_like(model.flat_params)
    assert lib.m2t_backward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(x), _lib.ptr(grads), ws, st) == STATE
    # a deferred request of any kind leaves no materialised seed for m2t_add_output_grad; an immediate one does
    g = torch.zeros(B, 3, 64, 64, device="cuda")
    for kind, param in ((1, 0.0), (2, 1e-6), (3, BETA)):
        assert call(lib.m2t_pixel_loss_deferred, kind, param) == 0
        assert lib.m2t_add_output_grad(plan.handle, _lib.ptr(g), 64, 64, None, 1.0, 1.0, ws, st) == STATE
        assert call(lib.m2t_pixel_loss, kind, param) == 0
        assert lib.m2t_add_output_grad(plan.handle, _lib.ptr(g), 64, 64, None, 1.0, 1.0, ws, st) == 0
    torch.cuda.synchronize()
