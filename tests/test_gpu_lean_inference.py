"""-m gpu: inference plans (option "inference" of include/m2t.h) against training plans, bit for bit.

An inference plan launches the kernels a training plan launches, in the same order, on a workspace where X1 .. X<n> rotate through two
buffers, every block shares one set of regions and the regions nothing reads in the forward are absent (null pointers).  So there is
no tolerance anywhere in this file: every comparison is torch.equal.

Shapes are the smallest at which the layout can go wrong: (1, 18, 24) is one C = 256 window, reflect-padded to 32 x 32; (2, 40, 56) is
non-square and padded to 64 x 64; (1, 96, 160) has an odd 3 x 5 window grid at the C = 256 level.  Depths 1 / 2 / 3: odd and even depths
catch a wrong ping-pong, depth 3 catches X0 aliased to a rotating buffer.  No test here needs the CPU oracle."""
import ctypes as C
import functools

import pytest
import torch

from oracle import m2trans_oracle as O
from tests.gpu_util import WS_PERSISTENT, build_model

pytestmark = pytest.mark.gpu

SHAPES = ((1, 18, 24), (2, 40, 56), (1, 96, 160))
UNFUSED = {"fused_attn_fwd": 0, "fused_c16_fwd": 0, "fused_tail": 0}
SETTINGS = (("default", {}), ("unfused", UNFUSED))
ERR_STATE = -3


@functools.lru_cache(maxsize=None)
def _model(scale, nb, dtype):
    return build_model(scale, nb, dtype)[0]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """Three different inputs of one shape, computed once."""
    B, H, W = shape
    return tuple(O.closed_form_image(B, 3, H, W, phase=0.37 + 0.91 * k).cuda() for k in range(3))


def _plan(model, shape, inference, options=None):
    from m2trans_amd.M2Trans_network import Plan
    B, H, W = shape
    return Plan(B, H, W, model.scale, model.n_blocks, model._dtype_code(), model.flat_params.device, inference=inference, options=options)


def _poison_all_but_persistent(plan):
    """0xFF (NaN as bf16 and as fp32) into every byte of the workspace outside the regions m2t_plan_init_workspace writes: the first
    three of WS_PERSISTENT (the fourth, red_descs, belongs to the backward pass: an inference plan has none)."""
    keep = torch.zeros(plan.workspace.numel(), dtype=torch.bool, device=plan.workspace.device)
    for n in WS_PERSISTENT[:3]:
        off, nbytes = plan.query("ws:" + n), plan.query("wsn:" + n)
        keep[off:off + nbytes] = True
    plan.workspace.masked_fill_(~keep, 0xFF)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("nb", (1, 2, 3))
@pytest.mark.parametrize("dtype", ("bf16", "fp32"))
@pytest.mark.parametrize("scale", (2, 3, 4))
def test_sr_is_bit_identical_and_independent_of_the_workspace_history(scale, dtype, nb, shape):
    """The inference plan's SR equals the training plan's under the default options and under the unfused kernels; three different
    inputs in a row on ONE inference plan equal the training plan's outputs; and so they do with every non-persistent byte of the
    workspace set to NaN between the calls (every region is written before it is read within one call, include/m2t.h)."""
    model = _model(scale, nb, dtype)
    xs = _inputs(shape)
    for tag, opts in SETTINGS:
        train, lean = _plan(model, shape, False, opts), _plan(model, shape, True, opts)
        assert lean.inference and lean.query("opt:inference") == 1 and train.query("opt:inference") == 0
        assert lean.workspace.numel() == lean.query("workspace_bytes") < train.query("workspace_bytes")
        for k in ("fused_attn_fwd", "fused_c16_fwd", "fused_tail"):
            assert lean.query("opt:" + k) == train.query("opt:" + k)
        want = [model._run_forward(train, x, keep=False) for x in xs]
        assert all(bool(torch.isfinite(w).all()) for w in want) and not torch.equal(want[0], want[1])
        for k, x in enumerate(xs):
            got = model._run_forward(lean, x, keep=False)
            assert torch.equal(got, want[k]), f"{tag}: input {k}: max |diff| {float((got - want[k]).abs().max())}"
        for k, x in enumerate(xs):
            _poison_all_but_persistent(lean)
            got = model._run_forward(lean, x, keep=False)
            assert torch.equal(got, want[k]), f"{tag}: input {k} after NaN in the workspace: a region is read before it is written"
        del train, lean


OTHER_SETTINGS = ({"fused_prep_fwd": 0}, {"fused_attn_fwd2": 1}, {"fused_attn_fwd2": 2}, {"fused_attn_fwd": 1, "fused_c16_fwd": 1},
                  {"fused_tail": 2}, {"fused_tail": 1}, {"conv_rows": 0}, {"fused_attn_fwd": 0}, {"fused_c16_fwd": 0})


@pytest.mark.parametrize("opts", OTHER_SETTINGS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("scale", (2, 4))
def test_other_option_settings_are_bit_identical_too(scale, opts):
    """Every option that changes which forward kernels run or what they store, one at a time, at (2, 40, 56), bf16, 3 blocks: the set
    of absent regions differs from setting to setting (q | k | v of the C = 256 branches is null on the fused path without branch_prep
    inside, present under the two-windows-per-CU kernels, ...)."""
    shape = (2, 40, 56)
    model = _model(scale, 3, "bf16")
    xs = _inputs(shape)
    train, lean = _plan(model, shape, False, opts), _plan(model, shape, True, opts)
    for k, v in opts.items():
        assert lean.query("opt:" + k) == train.query("opt:" + k)
    for k, x in enumerate(xs[:2]):
        want = model._run_forward(train, x, keep=False)
        _poison_all_but_persistent(lean)
        assert torch.equal(model._run_forward(lean, x, keep=False), want), f"input {k}"


def test_every_state_refusal_comes_before_any_launch():
    """LR (1, 48, 64) at x4 (SR 192 x 256: a size every loss entry takes, so that no argument rule answers first)."""
    from m2trans_amd import _lib
    lib = _lib.load()
    shape, scale = (1, 48, 64), 4
    model = _model(scale, 1, "bf16")
    x = O.closed_form_image(*shape[:1], 3, *shape[1:], phase=0.2).cuda()
    train, lean = _plan(model, shape, False), _plan(model, shape, True)
    want = model._run_forward(train, x, keep=False)
    err = lambda: lib.m2t_last_error_string().decode()

    def refused(rc):
        assert rc == ERR_STATE and "inference plan" in err(), (rc, err())

    # the option is frozen once the workspace is initialised -- on both kinds of plan; an inference plan takes no other option either
    refused(lib.m2t_set_option(lean.handle, b"inference", 0))
    refused(lib.m2t_set_option(lean.handle, b"inference", 1))
    refused(lib.m2t_set_option(train.handle, b"inference", 1))
    for k in ("fused_tail", "fused_attn_fwd", "side_stream", "conv_rows"):
        refused(lib.m2t_set_option(lean.handle, k.encode(), 0))
    assert lean.query("opt:inference") == 1 and train.query("opt:inference") == 0 and lean.query("opt:fused_tail") == 3
    assert lib.m2t_set_option(train.handle, b"fused_tail", 3) == 0          # a training plan still takes options

    st = _lib.stream_ptr()
    ws, par = _lib.ptr(lean.workspace), _lib.ptr(model.flat_params)
    Hs, Ws = shape[1] * scale, shape[2] * scale
    hr = torch.rand(1, 3, Hs, Ws, device="cuda")
    sr = torch.full((1, 3, Hs, Ws), -7.0, device="cuda")
    loss = torch.full((1,), -7.0, device="cuda")
    grads = torch.full_like(model.flat_params, -7.0)
    gx = torch.full_like(x, -7.0)
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    vgg = C.c_void_p()
    assert lib.m2t_vgg_create(C.byref(vgg), _lib.BF16) == 0
    taps = (C.c_double * 5)(1, 1, 1, 1, 1)
    lo, hi = (C.c_double * 2)(0.5, 0.5), (C.c_double * 2)(0.5, -0.5)
    p = lambda t: _lib.ptr(t)

    def calls():
        h = lean.handle
        yield lib.m2t_forward(h, par, p(x), p(sr), 1.0, 1, ws, st)
        yield lib.m2t_l1_loss(h, p(hr), 1.0, 1.0, 1.0, p(loss), ws, st)
        yield lib.m2t_l1_loss_deferred(h, p(hr), 1.0, 1.0, 1.0, p(loss), ws, st)
        yield lib.m2t_pixel_loss(h, 1, 0.0, p(hr), 1.0, 1.0, 1.0, p(loss), ws, st)
        yield lib.m2t_pixel_loss_deferred(h, 2, 1e-6, p(hr), 1.0, 1.0, 1.0, p(loss), ws, st)
        yield lib.m2t_ssim_loss(h, p(hr), 1.0, 1.0, 1.0, p(loss), 0, p(scratch), ws, st)
        yield lib.m2t_msssim_loss(h, p(hr), 1.0, 1.0, 1.0, p(loss), 0, p(scratch), ws, st)
        yield lib.m2t_vif_loss(h, p(hr), 1.0, 1.0, 1.0, 2.0, p(loss), 0, p(scratch), ws, st)
        yield lib.m2t_gmsd_loss(h, p(hr), 1.0, 1.0, 1.0, p(loss), 0, p(scratch), ws, st)
        yield lib.m2t_fft_loss(h, p(hr), 1.0, 1.0, 1.0, 0, p(loss), 0, p(scratch), ws, st)
        yield lib.m2t_wavelet_loss(h, p(hr), 1.0, 1.0, 1.0, lo, hi, 2, 1, None, 0.0, p(loss), 0, p(scratch), ws, st)
        yield lib.m2t_consistency_loss(h, p(x), 1.0, 1.0, 1.0, 0.0, p(loss), 0, p(scratch), ws, st)
        yield lib.m2t_vgg_loss(h, vgg, p(hr), 1.0, 1.0, 1.0, 0, 0.0, taps, p(loss), 0, p(scratch), ws, st)
        yield lib.m2t_set_output_grad(h, p(hr), 1.0, ws, st)
        yield lib.m2t_add_output_grad(h, p(hr), Hs, Ws, None, 1.0, 1.0, ws, st)
        yield lib.m2t_backward(h, par, p(x), p(grads), ws, st)
        yield lib.m2t_backward_ex(h, par, p(x), p(grads), p(gx), None, ws, st)
        yield lib.m2t_stream_wait_bucket(h, 0, st)

    try:
        for after_forward in (False, True):
            if after_forward:      # "after an inference forward the plan has neither activations nor a seed"
                assert torch.equal(model._run_forward(lean, x, keep=False), want)
            torch.cuda.synchronize()
            before = lean.workspace.clone()
            n = 0
            for rc in calls():
                refused(rc)
                n += 1
            assert n == 18
            torch.cuda.synchronize()
            assert torch.equal(lean.workspace, before), "a refused call wrote into the workspace"
            for t in (sr, loss, grads, gx):
                assert bool((t == -7.0).all()), "a refused call wrote an output"
    finally:
        lib.m2t_vgg_destroy(vgg)
    # a following valid forward still gives the right bits
    assert torch.equal(model._run_forward(lean, x, keep=False), want)
    with pytest.raises(_lib.M2TError, match="inference plan"):
        model._run_forward(lean, x, keep=True)


@pytest.mark.parametrize("dtype", ("bf16", "fp32"))
def test_module_with_lean_inference_gives_the_default_bits_and_still_trains(dtype):
    scale, nb, shape = 4, 2, (2, 40, 56)
    model, params = build_model(scale, nb, dtype)
    x = _inputs(shape)[0]
    with torch.no_grad():
        want = model(x)
    assert list(model._plans) == [(2, 40, 56, model._dtype_code(), x.device.index)]
    assert model.lean_inference() is model
    with torch.no_grad():
        got = model(x)
    assert torch.equal(got, want)
    key = (2, 40, 56, model._dtype_code(), x.device.index, "inference")
    assert list(model._plans)[-1] == key and len(model._plans) == 2
    lean = model._plans[key]
    assert lean.inference and lean.workspace.numel() == lean.query("workspace_bytes")
    assert lean.workspace.numel() < 0.5 * model._plans[key[:5]].workspace.numel()
    # a forward with an autograd edge keeps using the training plan, and its backward works
    ref, _ = build_model(scale, nb, dtype, params=params)
    outs = []
    for m in (model, ref):
        sr = m(x)
        assert sr.requires_grad
        sr.square().mean().backward()
        outs.append((sr.detach(), torch.cat([p.grad.reshape(-1) for _, p in m._trainable()])))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][0], want) and torch.equal(outs[0][1], outs[1][1])
    assert len(model._plans) == 2 and model._plans[key[:5]].trained and not lean.trained
    # no_grad with the flag off again: the training plan
    model.lean_inference(False)
    gen = lean.gen
    with torch.no_grad():
        assert torch.equal(model(x), want)
    assert lean.gen == gen


def test_a_lean_eval_forward_between_two_train_steps_changes_nothing():
    from m2trans_amd.train_step import TrainStep
    scale, nb, shape = 4, 2, (2, 40, 56)
    m_a, params = build_model(scale, nb, "bf16")
    m_b, _ = build_model(scale, nb, "bf16", params=params)
    m_a.lean_inference()
    ts_a, ts_b = TrainStep(m_a, lr=1e-3), TrainStep(m_b, lr=1e-3)
    xs = _inputs(shape)
    hrs = [O.closed_form_image(shape[0], 3, shape[1] * scale, shape[2] * scale, phase=0.7 + k).cuda() for k in range(2)]
    losses = []
    for k in range(2):
        losses.append((ts_a.step(xs[k], hrs[k]).clone(), ts_b.step(xs[k], hrs[k]).clone()))
        if k == 0:
            with torch.no_grad():
                sr_a, sr_b = m_a(xs[2]), m_b(xs[2])        # arm A: on an inference plan; arm B: on the training plan itself
            assert torch.equal(sr_a, sr_b)
    torch.cuda.synchronize()
    assert len(m_a._plans) == 2 and len(m_b._plans) == 1
    for la, lb in losses:
        assert torch.equal(la, lb)
    assert torch.equal(m_a.flat_params, m_b.flat_params)
    assert torch.equal(ts_a.exp_avg, ts_b.exp_avg) and torch.equal(ts_a.exp_avg_sq, ts_b.exp_avg_sq)
    assert not torch.equal(m_a.flat_params, build_model(scale, nb, "bf16", params=params)[0].flat_params)


def test_self_ensemble_and_tiled_inherit_the_flag():
    from m2trans_amd import infer
    model, _ = build_model(2, 2, "bf16")
    x = _inputs((1, 96, 160))[1]
    with torch.no_grad():
        want_e, want_s = infer.self_ensemble(model, x[:, :, :40, :56].contiguous(), with_spread=True)
        want_t = infer.tiled(model, x, 64, 16, tile_batch=4)
    n_train = len(model._plans)
    model.lean_inference()
    with torch.no_grad():
        got_e, got_s = infer.self_ensemble(model, x[:, :, :40, :56].contiguous(), with_spread=True)
        got_t = infer.tiled(model, x, 64, 16, tile_batch=4)
    assert torch.equal(got_e, want_e) and torch.equal(got_s, want_s) and torch.equal(got_t, want_t)
    lean = [k for k in model._plans if k[-1] == "inference"]
    assert lean and len(model._plans) == n_train + len(lean)


def test_the_command_line_and_upscale_folder_write_the_same_files_with_lean(tmp_path, capsys):
    """`python -m m2trans_amd.infer ... --lean` in process, and `upscale_folder(lean=True)`, which leaves the model's own flag alone."""
    import json

    import numpy as np
    import yaml
    from PIL import Image
    from m2trans_amd import infer
    model = _model(2, 1, "bf16")
    torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, tmp_path / "m.pt")
    with open(tmp_path / "c.yml", "w") as f:
        yaml.safe_dump({"model": "M2Trans", "scale": 2, "n_blocks": 1, "n_feats": 64, "colors": 3, "rgb_range": 1.0, "compute_dtype": "bf16"}, f)
    (tmp_path / "in").mkdir()
    Image.fromarray(np.random.default_rng(5).integers(0, 256, size=(24, 40, 3), dtype=np.uint8)).save(tmp_path / "in" / "img.png")
    argv = ["--config", str(tmp_path / "c.yml"), "--model_path", str(tmp_path / "m.pt"), "--input", str(tmp_path / "in")]
    assert infer.main(argv + ["--output", str(tmp_path / "plain")]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["lean"] is False
    assert infer.main(argv + ["--output", str(tmp_path / "lean"), "--lean"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["lean"] is True
    want = np.asarray(Image.open(tmp_path / "plain" / "img.png"))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "lean" / "img.png")), want)
    n = len(model._plans)
    assert infer.upscale_folder(model, tmp_path / "in", tmp_path / "lean2", lean=True) == ["img.png"]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "lean2" / "img.png")), want)
    assert model.lean_inference_enabled is False
    assert [k[-1] for k in list(model._plans)[n:]] == ["inference"]
