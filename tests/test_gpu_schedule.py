"""-m gpu: the race and stale-read gate of the two-stream training step.

m2t_backward puts every parameter-gradient kernel on a plan-owned side stream and orders the two streams with hand-placed events;
its buffers are double-buffered on the assumption that the side stream lags the main chain by at most two blocks.  With
``side_stream = 0`` the SAME kernels run with the same arguments in the same order on one stream, and no kernel of the step uses
atomics, so three invariants hold without any tolerance:

  1. the two-stream step equals the one-stream step bit for bit, at every step of a run over changing batches (step 1 is the
     first-backward schedule, steps 2.. the steady state), at the depth (8 blocks) where the ``b + 2`` buffer hazards are live;
  2. the same under partial / input-gradient passes (m2t_backward_ex) and under the pass that follows a partial one;
  3. a step's result does not depend on what the workspace held before it: NaN in every floating-point region, on a fresh plan
     and in steady state, changes no bit.

A failure names the step and the parameter tensors whose values differ: the stage they belong to is the stage whose side-stream
launches miss a dependency (groups 1, 2) or read a region before anything wrote it in this step (group 3).  No test here needs
the CPU oracle."""
import ctypes as C

import pytest
import torch

from oracle import m2trans_oracle as O
from oracle import swin_oracle as S
from tests.gpu_util import (assert_flat_equal, build_model, poison_float_regions, poison_whole_workspace, set_options,
                            ws_float_regions)

pytestmark = pytest.mark.gpu

K_STEPS = 4          # step 1: first_backward schedule; 2..: steady state (head reduction on the main stream); batches differ
PLAIN_BF16 = dict(attn_bwd=0, fused_conv_bwd=0, fused_tail=0)


def _image(B, h, w, phase):
    """B different closed-form images; beyond four samples the CPU generator (float64 sines: 0.4 s for 32 x 3 x 512 x 512, more
    than the steps under test) is replaced by shifted copies of the first four, made on the device."""
    base = O.closed_form_image(min(B, 4), 3, h, w, phase=phase).cuda()
    if B <= 4:
        return base
    return torch.cat([torch.roll(base, shifts=(3 * g, 5 * g), dims=(2, 3)) for g in range((B + 3) // 4)])[:B].contiguous()


def _batch(B, H, W, scale, step):
    return _image(B, H, W, 0.37 * step), _image(B, H * scale, W * scale, 0.7 + 0.91 * step)


def _two_models(scale, nb, dtype, B, H, W, opts):
    """Arm A: `opts`; arm B: the same and side_stream = 0.  Options are set before the first step."""
    shape = torch.empty(B, 3, H, W, device="cuda")
    m_a, p = build_model(scale, nb, dtype)
    m_b, _ = build_model(scale, nb, dtype, params=p)
    assert torch.equal(m_a.flat_params, m_b.flat_params)
    plan_a = set_options(m_a, shape, **opts)
    plan_b = set_options(m_b, shape, **opts, side_stream=0)
    assert plan_a.query("opt:side_stream") == 1 and plan_b.query("opt:side_stream") == 0
    for k, v in opts.items():
        if k in ("gate_branch", "wgrad_big_tiles"):
            assert plan_a.query("opt:" + k) == v + 1000 and plan_b.query("opt:" + k) == v + 1000
    return m_a, m_b, plan_a, plan_b


def _compare_arms(step, ts_a, ts_b, loss_a, loss_b, extra=()):
    torch.cuda.synchronize()
    tag = f"step {step} (two-stream arm vs one-stream arm)"
    assert torch.equal(loss_a, loss_b), f"{tag}: loss {float(loss_a)!r} vs {float(loss_b)!r}"
    for name, a, b in extra:
        assert torch.equal(a, b), f"{tag}: {name} differs"
    assert bool(torch.isfinite(ts_a.grads).all()), f"{tag}: non-finite gradient"
    assert_flat_equal(ts_a.model, ts_a.grads, ts_b.grads, f"{tag}: gradients")
    assert_flat_equal(ts_a.model, ts_a.model.flat_params, ts_b.model.flat_params, f"{tag}: parameters")
    assert_flat_equal(ts_a.model, ts_a.exp_avg, ts_b.exp_avg, f"{tag}: exp_avg")
    assert_flat_equal(ts_a.model, ts_a.exp_avg_sq, ts_b.exp_avg_sq, f"{tag}: exp_avg_sq")


def _drive(ts_a, ts_b, scale, B, H, W, caller_stream=False, captions=None, sem=None):
    """K_STEPS consecutive TrainStep.step calls on different batches, the arms interleaved step by step, every state compared
    after every step.  caller_stream: the steps run on a non-default stream (as the benchmark does)."""
    stream = torch.cuda.Stream() if caller_stream else torch.cuda.current_stream()
    for step in range(K_STEPS):
        x, hr = _batch(B, H, W, scale, step)
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            out = []
            for ts, sl in ((ts_a, sem[0] if sem else None), (ts_b, sem[1] if sem else None)):
                torch.manual_seed(1000 + step)             # (the SemanticLoss crop origins come from the global CPU generator)
                loss = ts.step(x, hr, captions).clone()
                per = sl.last_per_sample.clone() if sl is not None else None
                clip = ts.clip_loss.clone() if sl is not None else None
                out.append((loss, per, clip))
        stream.synchronize()
        (la, pa, ca), (lb, pb, cb) = out
        extra = [("last_per_sample", pa, pb), ("clip_loss", ca, cb)] if sem else []
        _compare_arms(step, ts_a, ts_b, la, lb, extra)
        if step > 0:
            assert not torch.equal(la, first_loss), "the batches must differ from step to step"
        else:
            first_loss = la
    assert float(ts_a.grads.abs().max()) > 0


# ------------------------------------------------------------------ 1. two-stream == one-stream, several steps, changing batches
SCHEDULE_CASES = [
    # id, dtype, scale, n_blocks, B, H, W, options of both arms, non-default caller stream
    pytest.param("bf16", 4, 8, 16, 128, 128, {}, True, id="bench-geometry-b16"),                 # BASELINE.json configs[1]
    pytest.param("bf16", 4, 8, 32, 128, 128, {}, False, id="b32-big-wgrad-tiles"),               # per-GPU share of configs[3]
    pytest.param("fp32", 4, 8, 4, 128, 128, {}, False, id="fp32-parity-mode"),                   # plain kernels, most work on the side stream
    pytest.param("bf16", 3, 8, 2, 256, 256, {}, False, id="x3-256-streaming-tail"),              # configs[4] geometry
    pytest.param("bf16", 2, 4, 4, 40, 56, {}, True, id="x2-40x56-reflect-padded"),               # windows on every border
    pytest.param("bf16", 4, 4, 4, 128, 128, PLAIN_BF16, False, id="plain-bf16-kernels"),         # halo gather + conv wgrad on the side stream
    pytest.param("bf16", 4, 4, 4, 128, 128, dict(gate_branch=0, fork_on_kernel=0), False, id="gate0-recorded-forks"),
    pytest.param("bf16", 4, 4, 4, 128, 128, dict(gate_branch=2, fork_on_kernel=0), False, id="gate2-recorded-forks"),
]


@pytest.mark.parametrize("dtype,scale,nb,B,H,W,opts,caller_stream", SCHEDULE_CASES)
def test_two_stream_step_equals_one_stream_step_at_every_step(dtype, scale, nb, B, H, W, opts, caller_stream):
    """Loss, gradients, parameters and both Adam moments, torch.equal after every one of K_STEPS steps."""
    from m2trans_amd.train_step import TrainStep
    m_a, m_b, plan_a, _ = _two_models(scale, nb, dtype, B, H, W, opts)
    if B >= 32 and dtype == "bf16":
        assert plan_a.query("opt:wgrad_big_tiles") == 999      # auto: the 128 x 128 tiles switch themselves on from 24 576 rows
    ts_a = TrainStep(m_a, lr=1e-3, world_size=1)
    ts_b = TrainStep(m_b, lr=1e-3, world_size=1)
    _drive(ts_a, ts_b, scale, B, H, W, caller_stream=caller_stream)


def test_communication_stream_live_equals_one_stream_step():
    """Arm A: the bucketed exchange path with one rank (bucket events, communication stream, Adam behind it), default options.
    Arm B: side_stream = 0 and no bucket.  Benchmark geometry (batch 16, 8 blocks): the full-depth steady state."""
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H, W = 4, 8, 16, 128, 128
    m_a, m_b, _, _ = _two_models(scale, nb, "bf16", B, H, W, {})
    ts_a = TrainStep(m_a, lr=1e-3, world_size=1, force_comm_path=True)
    ts_b = TrainStep(m_b, lr=1e-3, world_size=1)
    assert ts_a.overlap_comm and ts_a.comm_stream is not None and ts_b.bucket is None
    _drive(ts_a, ts_b, scale, B, H, W)


def _semantic(differentiable, B):
    from m2trans_amd.losses import SemanticLoss
    caps = [f"c{i}" for i in range(B)]
    g = torch.Generator().manual_seed(8)
    table = {c: torch.randn(512, generator=g) for c in caps}
    p = S.closed_form_swin_params()
    sls = []
    for _ in range(2):
        sl = SemanticLoss(criterion="l1", N_patches=3, device="cuda", compute_dtype="bf16", max_batch=B, differentiable=differentiable)
        sl.load_image_encoder(p)
        sl.set_text_features(table)
        sls.append(sl)
    return sls, caps


@pytest.mark.parametrize("differentiable", [False, True], ids=["constant-route", "differentiable-route"])
def test_semantic_loss_stream_live_equals_one_stream_step(differentiable):
    """configs[2]'s shape (x4, 128 x 128, 8 blocks, bf16) at batch 4, closed-form Swin-T weights, injected text features.
    Constant route: arm A runs the encoder on its own stream under the two-stream backward (overlap_semantic), arm B runs
    everything on one stream.  Differentiable route (m2t_l1_loss -> m2t_add_output_grad -> m2t_backward): side_stream 1 against 0.
    The same torch.manual_seed before each step on both arms; loss, clip_loss, last_per_sample and all state bit-identical."""
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H, W = 4, 8, 4, 128, 128
    m_a, m_b, _, _ = _two_models(scale, nb, "bf16", B, H, W, {})
    (sl_a, sl_b), caps = _semantic(differentiable, B)
    ts_a = TrainStep(m_a, lr=1e-3, world_size=1, semantic_loss=sl_a, lambda_clip=0.01, overlap_semantic=True)
    ts_b = TrainStep(m_b, lr=1e-3, world_size=1, semantic_loss=sl_b, lambda_clip=0.01, overlap_semantic=False)
    _drive(ts_a, ts_b, scale, B, H, W, captions=caps, sem=(sl_a, sl_b))
    assert float(sl_a.last_per_sample.sum()) > 0


# ------------------------------------------------------------------ 2. partial and input-gradient passes under both schedules
# (stages with requires_grad, input gradient wanted)
PASSES = [
    ("all", False),
    (("tail",), False),
    ((), True),                        # everything frozen: the data-gradient chain alone, no side-stream work
    (("head", "body.1"), True),
    (("head", "body.1"), True),        # the same mask again: its reduction table is re-used
    ("all", False),                    # the pass after a partial pass: the plan's published table, bucket events last recorded
    ("all", False),                    # "at the end of the whole pass"
]
SENTINEL = 123.0


def _stage_of(name):
    return ".".join(name.split(".")[:2]) if name.startswith("body.") else name.split(".")[0]


def _autograd_pass(model, x, w, stages, need_x):
    """The surface of tests/test_gpu_input_grad.py: requires_grad_ toggles select the stages, lr.requires_grad the input gradient."""
    for n, p in model._trainable():
        p.requires_grad_(stages == "all" or _stage_of(n) in stages)
    model.zero_grad(set_to_none=True)
    lr = x.detach().clone().requires_grad_(need_x)
    (model(lr) * w).sum().backward()
    torch.cuda.synchronize()
    grads = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in model._trainable()}
    return grads, (lr.grad.detach().clone() if need_x else None)


def _c_abi_pass(model, plan, x, w, stages, need_x, flat):
    """m2t_forward -> m2t_set_output_grad -> m2t_backward_ex into a caller-owned gradient buffer pre-filled with a sentinel."""
    from m2trans_amd import _lib
    lib = _lib.load()
    names = list(model.param_offsets())
    flags = model.stage_flags([stages == "all" or _stage_of(n) in stages for n in names])
    flat.fill_(SENTINEL)
    gx = torch.empty_like(x) if need_x else None
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(x), None, 1.0, 1, ws, st), "m2t_forward")
    _lib.check(lib.m2t_set_output_grad(plan.handle, _lib.ptr(w), 1.0, ws, st), "m2t_set_output_grad")
    cflags = (C.c_ubyte * len(flags))(*[1 if f else 0 for f in flags])
    _lib.check(lib.m2t_backward_ex(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(x), _lib.ptr(flat) if any(flags) else None,
                                   _lib.ptr(gx), cflags, ws, st), "m2t_backward_ex")
    torch.cuda.synchronize()
    grads = {}
    for n, (o, k) in model.param_offsets().items():
        wanted = stages == "all" or _stage_of(n) in stages
        grads[n] = flat[o:o + k].clone() if wanted else None
        if not wanted:
            assert bool((flat[o:o + k] == SENTINEL).all()), f"{n}: a range that was not requested lost its sentinel"
    return grads, gx


@pytest.mark.parametrize("surface", ["autograd", "c_abi"])
@pytest.mark.parametrize("dtype,B,H,W", [("bf16", 4, 128, 128), ("fp32", 2, 64, 64)])
def test_partial_and_input_gradient_passes_equal_under_both_schedules(dtype, B, H, W, surface):
    """One plan per arm (side_stream 1 against 0), 4 blocks, the fixed sequence PASSES on different batches: after every pass the
    requested parameter gradients and the input gradient are bit-identical between the arms; what was not requested is absent
    (autograd surface: p.grad is None) or keeps its sentinel (C ABI, caller-owned buffer)."""
    scale, nb = 4, 4
    m_a, m_b, plan_a, plan_b = _two_models(scale, nb, dtype, B, H, W, {})
    flats = [torch.empty_like(m.flat_params) for m in (m_a, m_b)]
    for i, (stages, need_x) in enumerate(PASSES):
        x = O.closed_form_image(B, 3, H, W, phase=0.37 * i).cuda()
        w = (O.closed_form_image(B, 3, H * scale, W * scale, phase=0.3 + 0.91 * i) - 0.45).cuda()
        res = []
        for model, plan, flat in ((m_a, plan_a, flats[0]), (m_b, plan_b, flats[1])):
            res.append(_autograd_pass(model, x, w, stages, need_x) if surface == "autograd"
                       else _c_abi_pass(model, plan, x, w, stages, need_x, flat))
        (g_a, gx_a), (g_b, gx_b) = res
        tag = f"pass {i + 1} (stages {stages}, gx {need_x})"
        bad = []
        for n in g_a:
            wanted = stages == "all" or _stage_of(n) in stages
            assert (g_a[n] is not None) == wanted and (g_b[n] is not None) == wanted, (tag, n)
            if wanted:
                assert bool(torch.isfinite(g_a[n]).all()), (tag, n)
                if not torch.equal(g_a[n], g_b[n]):
                    bad.append(n)
        assert not bad, f"{tag}: two-stream and one-stream gradients differ in {bad[:8]} ({len(bad)} tensors)"
        if need_x:
            assert bool(torch.isfinite(gx_a).all()) and float(gx_a.abs().max()) > 0, tag
            assert torch.equal(gx_a, gx_b), f"{tag}: input gradients differ"
        else:
            assert gx_a is None and gx_b is None


# ------------------------------------------------------------------ 3. history independence and poisoned workspace
POISON_CASES = [
    # dtype, scale, n_blocks, B, H, W, options
    pytest.param("bf16", 4, 4, 4, 128, 128, {}, id="bf16-x4-128"),
    pytest.param("bf16", 4, 4, 4, 40, 56, {}, id="bf16-x4-40x56"),
    pytest.param("fp32", 4, 4, 2, 64, 64, {}, id="fp32-x4"),                             # the deferred L1 seed kernel runs in m2t_backward
    pytest.param("bf16", 3, 4, 2, 64, 96, {}, id="bf16-x3"),
    pytest.param("bf16", 4, 4, 4, 128, 128, PLAIN_BF16, id="plain-bf16-kernels"),
    pytest.param("bf16", 4, 4, 4, 128, 128, dict(fused_l1=0), id="bf16-x4-seed-kernel"),  # ... and here (the bf16 path of that kernel)
]


def _fresh_step(model, x, hr, opts):
    """forward_backward on batch X on a fresh, untouched plan: (loss, gradients)."""
    from m2trans_amd.train_step import TrainStep
    model._plans.clear()
    set_options(model, x, **opts)
    ts = TrainStep(model, world_size=1)
    loss = ts.forward_backward(x, hr).clone()
    torch.cuda.synchronize()
    grads = ts.grads.clone()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0
    return loss, grads


def _assert_same_step(model, ts, loss, ref, what):
    torch.cuda.synchronize()
    ref_loss, ref_grads = ref
    assert bool(torch.isfinite(loss).all()), f"{what}: loss {float(loss)!r}"
    if not bool(torch.isfinite(ts.grads).all()):
        offs = model.param_offsets()
        bad = [n for n, (o, k) in offs.items() if not bool(torch.isfinite(ts.grads[o:o + k]).all())]
        raise AssertionError(f"{what}: non-finite gradients in {bad[:8]} ({len(bad)} tensors): a kernel read poisoned workspace")
    assert torch.equal(loss, ref_loss), f"{what}: loss {float(loss)!r} vs {float(ref_loss)!r} on an untouched fresh plan"
    assert_flat_equal(model, ts.grads, ref_grads, f"{what}: gradients vs an untouched fresh plan")


@pytest.mark.parametrize("dtype,scale,nb,B,H,W,opts", POISON_CASES)
def test_fresh_plan_with_a_poisoned_workspace_gives_the_same_step(dtype, scale, nb, B, H, W, opts):
    """(a) Whole workspace 0xFF (NaN as bf16 and as fp32), m2t_plan_init_workspace again, one forward_backward: finite, and
    bit-identical to the same call on an untouched fresh plan.  (The only index-carrying regions are pack_descs / pack_blocks,
    rewritten by m2t_plan_init_workspace, and red_descs, rewritten by the first backward pass after it: ws_float_regions checks
    that inventory against the library before anything is poisoned.)"""
    from m2trans_amd.train_step import TrainStep
    model, _ = build_model(scale, nb, dtype)
    x, hr = _batch(B, H, W, scale, 7)
    ref = _fresh_step(model, x, hr, opts)
    model._plans.clear()
    plan = set_options(model, x, **opts)
    poison_whole_workspace(plan)
    ts = TrainStep(model, world_size=1)
    loss = ts.forward_backward(x, hr)
    assert model._plan_for(x) is plan
    _assert_same_step(model, ts, loss, ref, "fresh plan, poisoned workspace")


@pytest.mark.parametrize("dtype,scale,nb,B,H,W,opts", POISON_CASES)
def test_steady_state_step_does_not_read_what_the_previous_steps_left(dtype, scale, nb, B, H, W, opts):
    """(b) Three forward_backward calls on batches A, B, C (no optimizer: the weights stay put), synchronise, 0xFF into every
    floating-point workspace region by name, then batch X: bit-identical to X on a fresh plan.  X runs the STEADY-STATE schedule
    (published reduction table, head reduction on the main stream), which a fresh plan never reaches."""
    from m2trans_amd.train_step import TrainStep
    model, _ = build_model(scale, nb, dtype)
    x, hr = _batch(B, H, W, scale, 7)
    ref = _fresh_step(model, x, hr, opts)
    model._plans.clear()
    plan = set_options(model, x, **opts)
    ts = TrainStep(model, world_size=1)
    for step in range(3):
        ts.forward_backward(*_batch(B, H, W, scale, step))
    torch.cuda.synchronize()
    poison_float_regions(plan)
    loss = ts.forward_backward(x, hr)
    assert model._plan_for(x) is plan
    _assert_same_step(model, ts, loss, ref, "steady state, poisoned between steps")


@pytest.mark.parametrize("dtype,scale,B,H,W", [("bf16", 4, 4, 128, 128), ("bf16", 2, 2, 40, 56), ("fp32", 4, 2, 64, 64)])
def test_forward_only_does_not_read_poisoned_workspace(dtype, scale, B, H, W):
    """eval / no_grad: sr of a poisoned plan (whole workspace + init; then every floating-point region by name on the live plan)
    against sr of an untouched fresh plan, bit for bit."""
    nb = 4
    model, _ = build_model(scale, nb, dtype)
    model.eval()
    x, _ = _batch(B, H, W, scale, 7)
    with torch.no_grad():
        ref = model(x).clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ref).all()) and float(ref.std()) > 0
        model._plans.clear()
        plan = model._plan_for(x)
        poison_whole_workspace(plan)
        got = model(x).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, ref), "fresh plan, poisoned workspace: sr differs"
        model(_batch(B, H, W, scale, 1)[0])
        torch.cuda.synchronize()
        poison_float_regions(plan)
        got = model(x).clone()
        torch.cuda.synchronize()
        assert model._plan_for(x) is plan
        assert torch.equal(got, ref), "live plan, poisoned between forwards: sr differs"


def test_workspace_region_inventory_is_complete():
    """The region list of the poison helper tiles the workspace of every plan kind used above (it raises otherwise), and the
    persistent regions hold what include/m2t.h says after m2t_plan_init_workspace."""
    for dtype, scale, nb, B, H, W in (("bf16", 4, 8, 2, 128, 128), ("fp32", 4, 4, 2, 64, 64), ("bf16", 3, 4, 1, 40, 56), ("fp32", 2, 1, 1, 32, 64)):
        model, _ = build_model(scale, nb, dtype)
        plan = model._plan_for(torch.empty(B, 3, H, W, device="cuda"))
        regions = ws_float_regions(plan)
        assert sum(n for _, _, n in regions) > 0.99 * plan.query("workspace_bytes")
        poison_whole_workspace(plan)
        torch.cuda.synchronize()
        off = plan.query("ws:zero_page")
        assert int(plan.workspace[off:off + 256].max()) == 0
