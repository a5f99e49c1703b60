"""-m gpu: the input gradient and the requires_grad-aware backward (m2t_backward_ex through the autograd node).
lr.grad against fp64 autograd through the oracle; bit-identity of every gradient that a frozen stage or an input gradient
must not change; the plan-state rules of partial passes; DataParallel; the guards."""
import ctypes as C

import pytest
import torch

from oracle import m2trans_oracle as O
from tests.gpu_util import build_model, rel, rms_rel

pytestmark = pytest.mark.gpu


def _weights(B, Hs, Ws):
    return (O.closed_form_image(B, 3, Hs, Ws, phase=0.3) - 0.45).cuda()


def _params(model):
    return [(n, p) for n, p in model._trainable()]


def _step(model, x, w=None, hr=None, need_x=True):
    """One forward + backward through autograd; returns (lr.grad, {name: grad or None}, sr)."""
    model.zero_grad(set_to_none=True)
    lr = x.detach().clone().requires_grad_(need_x)
    sr = model(lr)
    loss = (sr * w).sum() if w is not None else torch.nn.L1Loss()(sr, hr)
    loss.backward()
    torch.cuda.synchronize()
    g = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in _params(model)}
    return (lr.grad.detach().clone() if need_x else None), g, sr.detach()


def _set(model, x, **opts):
    from m2trans_amd import _lib
    plan = model._plan_for(x)
    for k, v in opts.items():
        _lib.check(_lib.load().m2t_set_option(plan.handle, k.encode(), int(v)), k)
    return plan


def _freeze(model, stages):
    """requires_grad only for the given stages: 'head', 'body.<b>', 'tail'."""
    for n, p in _params(model):
        st = n.split(".")[0] if not n.startswith("body.") else ".".join(n.split(".")[:2])
        p.requires_grad_(st in stages)


# ------------------------------------------------------------------ 1. fp32 lr.grad against fp64 autograd of the oracle
ORACLE_CASES = [(4, 1, 2, 32, 32), (2, 2, 1, 32, 64), (3, 1, 1, 32, 32), (4, 2, 1, 40, 56), (2, 1, 1, 33, 47)]


@pytest.mark.parametrize("scale,nb,B,H0,W0", ORACLE_CASES)
def test_input_grad_fp32_vs_fp64_oracle(scale, nb, B, H0, W0):
    model, p = build_model(scale, nb, "fp32")
    x = O.closed_form_image(B, 3, H0, W0)
    w = _weights(B, H0 * scale, W0 * scale)
    # an HR image that puts part of the output under the clamp: the L1 cotangent is masked there
    hr = (O.closed_form_image(B, 3, H0 * scale, W0 * scale, phase=0.7) * 1.2 - 0.1).clamp(0, 1).cuda()
    p64 = {k: v.double() for k, v in p.items()}
    for loss_kind in ("smooth", "l1"):
        xo = x.double().requires_grad_(True)
        so = O.forward(xo, p64, scale, nb)
        lo = (so * w.cpu().double()).sum() if loss_kind == "smooth" else (so - hr.cpu().double()).abs().mean()
        (go,) = torch.autograd.grad(lo, xo)
        gx, _, sr = _step(model, x.cuda(), w=w if loss_kind == "smooth" else None, hr=hr)
        assert gx.shape == x.shape and gx.dtype == torch.float32
        e = rel(gx, go)
        assert e <= 1e-4, (loss_kind, e)
        if loss_kind == "l1":
            assert bool(((sr <= 0) | (sr >= 1)).any())       # the clamp is live in this case


# ------------------------------------------------------------------ 2 / 3. bit-identity: the input gradient changes no parameter gradient; frozen model
def _full_and_frozen(dtype, scale, nb, B, H0, W0, **opts):
    model, _ = build_model(scale, nb, dtype)
    x = O.closed_form_image(B, 3, H0, W0).cuda()
    w = _weights(B, H0 * scale, W0 * scale)
    _set(model, x, **opts)
    _, g_ref, sr_ref = _step(model, x, w=w, need_x=False)           # m2t_backward (today's path)
    gx, g_x, sr = _step(model, x, w=w, need_x=True)                 # m2t_backward_ex, every stage + the input
    assert torch.equal(sr, sr_ref)
    for n in g_ref:
        assert torch.equal(g_x[n], g_ref[n]), n
    model.requires_grad_(False)
    flat_g = model.attach_flat_grads()
    flat_g.fill_(123.0)
    for _, p in _params(model):
        p.grad = None
    gx_f, g_f, sr_f = _step(model, x, w=w, need_x=True)              # frozen: lr.grad only
    assert torch.equal(sr_f, sr_ref)
    assert all(v is None for v in g_f.values())
    assert bool((flat_g == 123.0).all())
    assert torch.equal(gx_f, gx)
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    return gx


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_input_grad_changes_no_parameter_gradient_and_frozen_matches(dtype):
    _full_and_frozen(dtype, 4, 2, 2, 32, 32)


def test_frozen_bf16_every_fused_kernel_live():
    _full_and_frozen("bf16", 4, 2, 4, 128, 128)


@pytest.mark.parametrize("opts", [dict(attn_bwd=0), dict(fused_conv_bwd=0), dict(side_stream=0), dict(fused_tail=0)])
def test_frozen_matches_under_other_options(opts):
    _full_and_frozen("bf16", 4, 2, 2, 64, 64, **opts)
    _full_and_frozen("fp32", 2, 1, 1, 32, 64, **opts)


# ------------------------------------------------------------------ 4. partial masks
MASKS = [("tail",), ("body.1", "tail"), ("head",), ("head", "tail")]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_partial_masks_are_bit_identical_to_the_full_backward(dtype):
    scale, nb, B, H0, W0 = 4, 2, 2, 32, 64
    model, _ = build_model(scale, nb, dtype)
    x = O.closed_form_image(B, 3, H0, W0).cuda()
    w = _weights(B, H0 * scale, W0 * scale)
    gx_ref, g_ref, _ = _step(model, x, w=w, need_x=True)
    for stages in MASKS:
        for need_x in (False, True):
            _freeze(model, stages)
            gx, g, _ = _step(model, x, w=w, need_x=need_x)
            for (n, p) in _params(model):
                if p.requires_grad:
                    assert g[n] is not None and torch.equal(g[n], g_ref[n]), (stages, need_x, n)
                else:
                    assert g[n] is None, (stages, n)
            if need_x:
                assert torch.equal(gx, gx_ref), stages
            model.requires_grad_(True)


# ------------------------------------------------------------------ 5. plan state
def test_plan_state_across_full_frozen_partial_full():
    from m2trans_amd import _lib
    scale, nb, B, H0, W0 = 4, 2, 2, 32, 32
    model, _ = build_model(scale, nb, "bf16")
    x = O.closed_form_image(B, 3, H0, W0).cuda()
    w = _weights(B, H0 * scale, W0 * scale)
    _, g0, _ = _step(model, x, w=w, need_x=False)
    model.requires_grad_(False)
    gx_f, _, _ = _step(model, x, w=w, need_x=True)
    _freeze(model, ("body.0", "tail"))
    _step(model, x, w=w, need_x=False)
    _step(model, x, w=w, need_x=True)                                # the same mask again: its table is re-used
    plan = model._plan_for(x)
    # after a partial pass every bucket event marks its end: a stream that waits on any bucket sees the whole pass
    s2 = torch.cuda.Stream()
    lib = _lib.load()
    for i in range(plan.query("grad_buckets")):
        assert lib.m2t_stream_wait_bucket(plan.handle, i, C.c_void_p(s2.cuda_stream)) == 0
    model.requires_grad_(True)
    _, g1, _ = _step(model, x, w=w, need_x=False)
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    # a fresh plan whose first backward is partial, then a full one, equals a fresh full backward
    m2, _ = build_model(scale, nb, "bf16")
    _freeze(m2, ("tail",))
    _step(m2, x, w=w, need_x=True)
    m2.requires_grad_(True)
    _, g2, _ = _step(m2, x, w=w, need_x=False)
    for n in g0:
        assert torch.equal(g2[n], g0[n]), n


def test_stream_wait_bucket_after_a_partial_pass_waits_for_the_pass():
    """Documented rule: after a pass with some stage frozen every bucket event is recorded at the end of that pass, so a wait on
    any bucket -- the tail's, the first one, included -- orders the waiting stream behind the whole pass."""
    from m2trans_amd import _lib
    model, _ = build_model(4, 2, "fp32")
    x = O.closed_form_image(1, 3, 32, 32).cuda()
    w = _weights(1, 128, 128)
    _freeze(model, ("head",))
    model.zero_grad(set_to_none=True)
    plan = model._plan_for(x)
    s2 = torch.cuda.Stream()
    (model(x) * w).sum().backward()
    gh = model.head.weight.grad              # the head stage's range of the flat gradient buffer: the last one the pass writes
    with torch.cuda.stream(s2):
        assert _lib.load().m2t_stream_wait_bucket(plan.handle, 0, C.c_void_p(s2.cuda_stream)) == 0   # (the tail's bucket)
        seen = gh.clone()
    s2.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(seen, gh)
    for i in range(plan.query("grad_buckets")):
        assert _lib.load().m2t_stream_wait_bucket(plan.handle, i, C.c_void_p(s2.cuda_stream)) == 0
    s2.synchronize()


def test_train_step_after_partial_passes_is_unchanged():
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H0, W0 = 4, 1, 2, 32, 32
    x = O.closed_form_image(B, 3, H0, W0).cuda()
    hr = O.closed_form_image(B, 3, H0 * scale, W0 * scale, phase=0.7).cuda()
    w = _weights(B, H0 * scale, W0 * scale)
    outs = []
    for warm in (False, True):
        model, _ = build_model(scale, nb, "bf16")
        if warm:
            _freeze(model, ("tail",))
            _step(model, x, w=w, need_x=True)
            model.requires_grad_(False)
            _step(model, x, w=w, need_x=True)
            model.requires_grad_(True)
            model.zero_grad(set_to_none=True)
        ts = TrainStep(model, lr=1e-4, world_size=1)
        loss = ts.step(x, hr)
        torch.cuda.synchronize()
        outs.append((float(loss), model.flat_params.detach().clone()))
    assert outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------ 6. bf16 accuracy
def test_bf16_input_grad_vs_bf16_rounding_oracle():
    scale, nb, B, H0, W0 = 4, 1, 1, 32, 32
    model, p = build_model(scale, nb, "bf16")
    x = O.closed_form_image(B, 3, H0, W0)
    w = _weights(B, H0 * scale, W0 * scale)
    xo = x.clone().requires_grad_(True)
    so = O.forward(xo, p, scale, nb, emulate_bf16=True)
    (go,) = torch.autograd.grad((so * w.cpu()).sum(), xo)
    gx, _, _ = _step(model, x.cuda(), w=w)
    e = rms_rel(gx, go)
    assert e <= 2e-2, e


def test_bf16_input_grad_at_benchmark_geometry_close_to_fp32_mode():
    """x4, B = 16, 128^2, 8 blocks, frozen model: bf16 lr.grad against the HIP fp32 mode's."""
    x = torch.rand(16, 3, 128, 128, generator=torch.Generator().manual_seed(7)).cuda()
    w = _weights(16, 512, 512)
    got = {}
    for dtype in ("bf16", "fp32"):
        model, _ = build_model(4, 8, dtype)
        model.requires_grad_(False)
        got[dtype], _, _ = _step(model, x, w=w)
        del model
    a, b = got["bf16"].double().flatten(), got["fp32"].double().flatten()
    cos = float(a @ b / (a.norm() * b.norm()))
    assert cos >= 0.99, cos


# ------------------------------------------------------------------ 7. other input types
def test_channels_last_float64_and_sliced_inputs():
    model, _ = build_model(2, 1, "fp32")
    x = O.closed_form_image(2, 3, 32, 32).cuda()
    w = _weights(2, 64, 64)
    ref, _, _ = _step(model, x, w=w)
    model.requires_grad_(False)
    cl = x.detach().clone().to(memory_format=torch.channels_last).requires_grad_(True)
    (model(cl) * w).sum().backward()
    assert cl.grad.shape == x.shape and cl.grad.dtype == torch.float32 and torch.equal(cl.grad.contiguous(), ref)
    d = x.detach().double().requires_grad_(True)
    (model(d) * w).sum().backward()
    assert d.grad.dtype == torch.float64 and torch.equal(d.grad, ref.double())
    big = torch.zeros(2, 3, 40, 48, device="cuda")
    big[:, :, 4:36, 8:40] = x
    big.requires_grad_(True)
    (model(big[:, :, 4:36, 8:40]) * w).sum().backward()
    assert torch.equal(big.grad[:, :, 4:36, 8:40], ref)
    assert float(big.grad[:, :, :4].abs().max()) == 0.0 and float(big.grad[:, :, :, :8].abs().max()) == 0.0


# ------------------------------------------------------------------ 8. DataParallel
def test_data_parallel_input_grad_matches_the_single_module():
    import warnings
    import torch.nn as nn
    scale, nb, B, H, W = 4, 2, 4, 32, 64
    x = O.closed_form_image(B, 3, H, W).cuda()
    w = _weights(B, H * scale, W * scale)
    single, _ = build_model(scale, nb, "fp32")
    gx1, g1, _ = _step(single, x, w=w)
    multi, _ = build_model(scale, nb, "fp32")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dp = nn.DataParallel(multi, device_ids=[0, 0])
        for frozen in (False, True):
            multi.requires_grad_(not frozen)
            multi.zero_grad(set_to_none=True)
            lr = x.clone().requires_grad_(True)
            (dp(lr) * w).sum().backward()
            torch.cuda.synchronize()
            assert lr.grad is not None and rel(lr.grad, gx1) <= 2e-5, frozen
            if not frozen:
                assert all(rel(p.grad, g1[n]) < 2e-5 for n, p in _params(multi))
            else:
                assert all(p.grad is None for _, p in _params(multi))


# ------------------------------------------------------------------ 9. guards
def test_guards():
    from m2trans_amd._lib import M2TError
    model, _ = build_model(2, 1, "fp32")
    x = O.closed_form_image(1, 3, 32, 32).cuda()
    w = _weights(1, 64, 64)
    model.requires_grad_(False)
    # a backward after a later same-shape forward
    lr = x.clone().requires_grad_(True)
    sr = model(lr)
    with torch.no_grad():
        model(x)
    sr2 = model(x.clone().requires_grad_(True))
    with pytest.raises(M2TError):
        (sr * w).sum().backward()
    del sr2
    # second order
    lr = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((model(lr) * w).sum(), lr, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # no autograd node where no gradient can flow; same bits as the no-grad route
    with torch.no_grad():
        ref = model(x)
        assert model(x.clone().requires_grad_(True)).grad_fn is None
    out = model(x)
    assert out.grad_fn is None and torch.equal(out, ref)
    model.requires_grad_(True)
    with torch.no_grad():
        assert torch.equal(model(x.clone().requires_grad_(True)), ref)
