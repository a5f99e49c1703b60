"""-m gpu: option "local_norm" of include/m2t.h -- local-window InstanceNorm statistics (the Test-time Local Converter) on inference
plans -- against the numpy restatement of tests/local_norm_ref.py and against the oracle with its instance_norm replaced by it.

Where things are read from: the layout of an inference plan leaves the LAST block's input in place -- "ws:X<n_blocks - 1>" (X0 for one
block, X1 for two; from three blocks on X<n> aliases X<n - 2>, never X<n - 1>) -- and "ws:xn" holds that block's normalised input, so
the stage test compares the device's Xn with the restatement applied to the device's own X, teacher-forced, after a whole forward.

Shapes: (2, 40, 56) pads to a 64 x 64 plane, (1, 40, 88) to 64 x 96.  On those, T = 24 is even with an interior and both clamped
borders, 33 is odd, 64 is the plane, 200 is clipped to it, and 80 on 64 x 96 is global in rows and local in columns; 64 rows is one
row segment of the second pass, 64 / 96 columns are two / three column segments of the first.  The inputs are a ramp plus noise plus
a black half-plane, so that windows differ."""
import functools

import numpy as np
import pytest
import torch

from oracle import m2trans_oracle as O
from tests import local_norm_ref as R
from tests.gpu_util import _ws_p64, build_model, rel, rms_rel, ws_nchw
from tests.test_gpu_baseline_configs import STAGE_RMS

pytestmark = pytest.mark.gpu

ERR_STATE = -3
STAGE_CASES = tuple(((2, 40, 56), T) for T in (24, 33, 64, 200)) + (((1, 40, 88), 80),)
FP32_SR_BOUND = 1e-4        # tests/test_gpu_model.py:76, the fp32 forward against the oracle: rel(sr, oracle) < 1e-4


@functools.lru_cache(maxsize=None)
def _model(scale, nb, dtype):
    return build_model(scale, nb, dtype)


@functools.lru_cache(maxsize=None)
def _image(shape, seed=0):
    return torch.from_numpy(R.stage_input(*shape, seed=seed))


def _plan(model, shape, T=0, inference=True):
    from m2trans_amd.M2Trans_network import Plan
    B, H, W = shape
    kind = {"local_norm": T} if T else {}
    return Plan(B, H, W, model.scale, model.n_blocks, model._dtype_code(), model.flat_params.device, inference=inference, **kind)


def _padded(plan):
    return plan.query("padded_h"), plan.query("padded_w")


def _poison_and_reinitialise(plan):
    """What gpu_util.poison_whole_workspace does -- 0xFF into the WHOLE workspace, then m2t_plan_init_workspace again -- without its
    inventory check, which lists the regions of a training plan (on an inference plan most of them are absent by design)."""
    from m2trans_amd import _lib
    plan.workspace.fill_(0xFF)
    _lib.check(_lib.load().m2t_plan_init_workspace(plan.handle, _lib.ptr(plan.workspace), _lib.stream_ptr()), "m2t_plan_init_workspace")


# ------------------------------------------------------------------------------------------------------------------- a. stage
@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
@pytest.mark.parametrize("nb", (1, 2))
@pytest.mark.parametrize("shape,T", STAGE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"T{v}")
def test_stage_xn_against_the_restatement_on_the_devices_own_input(shape, T, nb, dtype):
    """Every element of Xn within 2^-22 (|x| + |m|) r (the four fp32 roundings of mean, difference, rstd and product, doubled) plus one
    rounding of the output type (2^-24 or 2^-8 relative) of the fp64 restatement applied to the block input the device itself stored.
    No element is excluded."""
    model, _ = _model(2, nb, dtype)
    plan = _plan(model, shape, T)
    assert plan.query("opt:local_norm") == T and plan.query("opt:inference") == 1
    sr = model._run_forward(plan, _image(shape).cuda(), keep=False)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sr).all())
    B = shape[0]
    H, W = _padded(plan)
    x = ws_nchw(plan, f"X{nb - 1}", B, H, W, 64).double().numpy()          # the last block's input, left in place
    xn = _ws_p64(plan, "xn", B, H, W).double().numpy()
    nbad, worst = R.gate(xn, x, T, dtype)
    m, v, r = R.local_stats_cumsum(x, T)
    print(f"{dtype} nb {nb} {shape} T {T}: worst |err| / bound {worst:.3f}, outside {nbad} of {xn.size}; r in [{r.min():.3g}, {r.max():.3g}], "
          f"{len(np.unique(m[0, 0]))} distinct window means in plane (0, 0)")
    assert len(np.unique(m[0, 0])) > 1 or T >= max(H, W)                 # windows do differ
    assert nbad == 0, (nbad, worst)
    # the identity record is what the consumers read
    ident = plan.ws_tensor("norm_id", dtype=torch.float32).view(2, B, 64)
    assert bool((ident[0] == 0).all()) and bool((ident[1] == 1).all())


# ------------------------------------------------------------------------------------------------------------- b. exact zeros
@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
@pytest.mark.parametrize("nb", (1, 2))
def test_an_all_black_input_gives_exact_zeros(nb, dtype):
    """A black image makes every block input constant per channel: X0 is the head bias; with xn = 0 the branches give 0 (q | k | v
    are products with 0, so the attention output is 0 whatever the softmax) and the zero-padded conv of 0 is its bias, so X1 is
    constant too.  On a constant c every sum the two passes form is j c for an integer j <= n <= 2^28: exact in fp64 (c has at
    most 24 significant bits), added or subtracted in any order.  So S1 = n c exactly, m = S1 / n = c exactly (a correctly rounded
    quotient of an exact one), mean32 = c, x - mean32 = +0 exactly, and +0 * rstd32 = +0: every BIT of Xn is zero."""
    shape, T = (2, 40, 56), 24
    model, _ = _model(2, nb, dtype)
    plan = _plan(model, shape, T)
    plan.ws_tensor("xn").fill_(1.0)
    model._run_forward(plan, torch.zeros(shape[0], 3, *shape[1:], device="cuda"), keep=False)
    torch.cuda.synchronize()
    xn = plan.ws_tensor("xn")
    bits = xn.view(torch.int32 if dtype == "fp32" else torch.int16)
    assert int((bits != 0).sum()) == 0
    x = plan.ws_tensor(f"X{nb - 1}").float()
    assert float(x.abs().max()) > 0                                       # (the block input itself is not zero: it is the bias)


# -------------------------------------------------------------------------------------------------------------- c. fp32 model
def _patched_norm(T, dtype):
    """oracle.instance_norm -> the restatement on the (N, C, H, W) plane cftm hands it; under the bf16 emulation Xn is rounded to bf16
    as the device stores it."""
    def norm(x, eps=1e-5):
        assert eps == 1e-5
        out = R.local_norm(x.detach().double().numpy(), T, dtype)
        return torch.from_numpy(out).to(x.dtype)
    return norm


@pytest.mark.parametrize("scale", (2, 3, 4))
def test_fp32_model_against_the_oracle_with_local_statistics(scale, monkeypatch):
    shape, T, nb = (1, 40, 56), 24, 2
    model, p = _model(scale, nb, "fp32")
    x = _image(shape)
    monkeypatch.setattr(O, "instance_norm", _patched_norm(T, "fp32"))
    with torch.no_grad():
        want = O.forward(x, p, scale, nb)
    monkeypatch.undo()
    plan = _plan(model, shape, T)
    sr = model._run_forward(plan, x.cuda(), keep=False)
    plain = model._run_forward(_plan(model, shape), x.cuda(), keep=False)
    e = rel(sr.cpu(), want)
    print(f"x{scale}: rel(sr, oracle with local statistics) {e:.3e}; local against global statistics {rel(sr, plain):.3e}")
    assert rel(sr, plain) > 1e-2                                          # the statistics do matter
    assert e < FP32_SR_BOUND


# -------------------------------------------------------------------------------------------------------------- d. bf16 model
@pytest.mark.parametrize("nb", (1, 2))
def test_bf16_model_against_the_emulating_oracle(nb, monkeypatch):
    """Teacher-forced on what an inference plan still holds after the forward: X0 .. X<nb>, the last block's xc and the d tensors
    its layout keeps, srpre.  Every tensor the oracle reports within STAGE_RMS of the device's."""
    scale, shape, T = 2, (1, 40, 56), 24
    model, p = _model(scale, nb, "bf16")
    x = _image(shape)
    plan = _plan(model, shape, T)
    sr = model._run_forward(plan, x.cuda(), keep=False)
    torch.cuda.synchronize()
    B = shape[0]
    H, W = _padded(plan)
    force = {f"X{b}": ws_nchw(plan, f"X{b}", B, H, W, 64) for b in range(nb + 1)}
    last = f"b{nb - 1}."
    force[last + "xc"] = ws_nchw(plan, last + "xc", B, H, W, 64)
    for i, (C, L) in enumerate(((16, 0), (64, 1), (256, 2), (256, 2))):
        try:
            force[f"{last}d{i + 1}"] = ws_nchw(plan, f"{last}d{i + 1}", B, H >> L, W >> L, C)
        except KeyError:
            pass                                                          # absent on this schedule
    force["srpre"] = plan.ws_tensor("srpre", dtype=torch.float32).view(B, 3, H * scale, W * scale).cpu().clone()
    rep = {}
    monkeypatch.setattr(O, "instance_norm", _patched_norm(T, "bf16"))
    with torch.no_grad():
        want = O.forward(x, p, scale, nb, emulate_bf16=True, force=force, stage_report=rep)
    monkeypatch.undo()
    for k, (mx, rms) in sorted(rep.items()):
        print(f"nb {nb}: {k:10s} max {mx:.3e} rel-rms {rms:.3e}")
    print(f"nb {nb}: sr rel-rms {rms_rel(sr.cpu(), want):.3e}")
    assert {f"X{b}" for b in range(nb + 1)} <= set(rep) and "srpre" in rep
    bad = {k: v for k, v in rep.items() if not v[1] < STAGE_RMS}
    assert not bad, bad
    assert rms_rel(sr.cpu(), want) < STAGE_RMS


# ---------------------------------------------------------------------------------------------------------- e. reproducibility
@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_bits_repeat_survive_a_poisoned_workspace_and_do_not_depend_on_the_batch(dtype):
    scale, nb, T = 2, 2, 24
    model, _ = _model(scale, nb, dtype)
    x3 = torch.cat([_image((1, 40, 56), seed=s) for s in range(3)]).cuda()
    plan = _plan(model, (3, 40, 56), T)
    H, W = _padded(plan)
    a = model._run_forward(plan, x3, keep=False)
    xn_a = plan.ws_tensor("xn").clone()
    b = model._run_forward(plan, x3, keep=False)
    assert torch.equal(a, b) and torch.equal(plan.ws_tensor("xn"), xn_a), "two runs differ"
    # 0xFF over everything, the persistent regions included; m2t_plan_init_workspace alone re-establishes them
    _poison_and_reinitialise(plan)
    ident = plan.ws_tensor("norm_id", dtype=torch.float32).view(2, 3, 64)
    assert bool((ident[0] == 0).all()) and bool((ident[1] == 1).all())
    c = model._run_forward(plan, x3, keep=False)
    assert torch.equal(a, c) and torch.equal(plan.ws_tensor("xn"), xn_a), "the forward reads something it did not write"
    # image b of the batch against the same image alone
    one = _plan(model, (1, 40, 56), T)
    xn3 = xn_a.view(4, 3, H * W * 16)
    for i in range(3):
        alone = model._run_forward(one, x3[i:i + 1].contiguous(), keep=False)
        assert torch.equal(one.ws_tensor("xn").view(4, 1, H * W * 16)[:, 0], xn3[:, i]), f"Xn of image {i} depends on the batch"
        assert torch.equal(alone[0], a[i]), f"sr of image {i} depends on the batch"


def test_the_option_is_frozen_once_the_workspace_is_initialised():
    from m2trans_amd import _lib
    lib = _lib.load()
    model, _ = _model(2, 1, "bf16")
    lean, ln = _plan(model, (1, 40, 56)), _plan(model, (1, 40, 56), 24)
    for plan, v in ((lean, 24), (ln, 0), (ln, 96)):
        assert lib.m2t_set_option(plan.handle, b"local_norm", v) == ERR_STATE
        assert "m2t_plan_init_workspace" in lib.m2t_last_error_string().decode()
    assert lean.query("opt:local_norm") == 0 and ln.query("opt:local_norm") == 24


# ------------------------------------------------------------------------------------------------------------------ f. surface
def test_model_local_norm_is_the_hand_made_plan_and_autograd_keeps_global_statistics():
    scale, nb, shape, T = 2, 2, (2, 40, 56), 24
    model, params = build_model(scale, nb, "bf16")
    ref, _ = build_model(scale, nb, "bf16", params=params)
    x = _image(shape).cuda()
    hand = model._run_forward(_plan(model, shape, T), x, keep=False)
    lean_want = model._run_forward(_plan(model, shape, 0, inference=False), x, keep=False)
    with torch.no_grad():
        plain = ref(x)
        assert model.local_norm(T) is model
        got = model(x)
    assert torch.equal(got, hand) and not torch.equal(got, plain)
    assert torch.equal(plain, lean_want)
    # the plain inference plan's sr is what it was: the training plan's
    assert torch.equal(model._run_forward(_plan(model, shape), x, keep=False), plain)
    key = (2, 40, 56, model._dtype_code(), x.device.index, "local_norm", T)
    assert list(model._plans) == [key] and model._plans[key].query("opt:local_norm") == T
    # under autograd: the ordinary training plan, global statistics -- train global, test local
    sr = model(x)
    assert sr.requires_grad and torch.equal(sr.detach(), plain)
    sr.square().mean().backward()
    assert len(model._plans) == 2
    with torch.no_grad():
        assert torch.equal(model.local_norm(0)(x), plain)


def test_the_inference_helpers_run_with_it(tmp_path):
    from m2trans_amd import infer, metrics
    scale, T = 2, 24
    model, _ = build_model(scale, 1, "bf16")
    x = _image((1, 96, 160)).cuda()
    small = x[:, :, :40, :56].contiguous()
    with torch.no_grad():
        plain_t = infer.tiled(model, x, 64, 16, tile_batch=4)
        plain_e = infer.self_ensemble(model, small)
        model.local_norm(T)
        got_t = infer.tiled(model, x, 64, 16, tile_batch=4)
        got_e = infer.self_ensemble(model, small)
        hr = torch.rand(1, 3, 40 * scale, 56 * scale, device="cuda")
        scores = metrics.evaluate(model, [(small, hr)], scale)
    assert got_t.shape == plain_t.shape and bool(torch.isfinite(got_t).all()) and not torch.equal(got_t, plain_t)
    assert got_e.shape == plain_e.shape and bool(torch.isfinite(got_e).all()) and not torch.equal(got_e, plain_e)
    assert len(scores) == 2 and all(np.isfinite(s) for s in scores)
    assert any(k[5:] == ("local_norm", T) for k in model._plans)


def test_upscale_folder_writes_the_bytes_of_the_hand_composition(tmp_path):
    from PIL import Image
    from m2trans_amd import infer
    T = 24
    model, _ = build_model(2, 1, "bf16")
    (tmp_path / "in").mkdir()
    u8 = (R.stage_input(1, 40, 56, seed=5)[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    Image.fromarray(u8).save(tmp_path / "in" / "img.png")
    assert infer.upscale_folder(model, tmp_path / "in", tmp_path / "a", local_norm=T) == ["img.png"]
    assert model.local_norm_window == 0 and model.lean_inference_enabled is False      # the model's own setting is left alone
    lr = infer.load_image(tmp_path / "in" / "img.png", "cuda")
    infer.save_image(model._run_forward(_plan(model, (1, 40, 56), T), lr, keep=False), tmp_path / "hand.png")
    assert (tmp_path / "a" / "img.png").read_bytes() == (tmp_path / "hand.png").read_bytes()
    assert infer.upscale_folder(model, tmp_path / "in", tmp_path / "b") == ["img.png"]
    assert (tmp_path / "b" / "img.png").read_bytes() != (tmp_path / "a" / "img.png").read_bytes()
