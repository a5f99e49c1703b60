"""CPU tests (no GPU) of the LR-consistency family (include/m2t_consistency.h): the C ABI table, the fp64 restatement the GPU tests
compare the kernels with (tests/consistency_ref.py) -- D against tests/imresize_ref.py, the dot-product identity of its adjoint, its
gradient against torch autograd through the dense matrices --, the spectrum that makes back-projection a contraction, the monotone fall
of the residual maximum for the inputs the GPU test uses, TrainStep's arguments and call sequence, the checkpoint keys, train.py's keys
and its refusal next to `degradation:`, the command line, and the kernel text run on host threads (tests/consistency_emulate.cpp) under
the gate of the GPU test."""
import contextlib
import ctypes as C
import inspect
import os
import re
import shutil
import struct
import types

import numpy as np
import pytest
import torch

from tests import consistency_ref as CR
from tests import imresize_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_decide_sizes_and_bad_arguments_on_the_host():
    from m2trans_amd import _lib
    lib = _lib.load()
    sb = lib.m2t_consistency_scratch_bytes
    assert sb(1, 1, 1, 1, 2) == 8 * (1 + 4) and sb(2, 3, 16, 32, 4) == 8 * (6 * 16 * 32 + 6 * 4) and sb(2, 3, 17, 33, 3) == 8 * (6 * 17 * 33 + 6 * 4 * 4)
    for bad in ((0, 3, 4, 4, 2), (1, 2, 4, 4, 2), (1, 3, 0, 4, 2), (1, 3, 4, 0, 2), (1, 3, 4, 4, 1), (1, 3, 4, 4, 5), (21846, 3, 4, 4, 2),
                (1, 3, 8193, 4, 2), (1, 3, 4, 4097, 4)):
        assert sb(*bad) == 0, bad
    one = C.c_void_p(8)                                              # a non-null pointer that is never followed
    call = lambda **kw: lib.m2t_consistency_loss_tensor(*[kw.get(k, v) for k, v in (
        ("x", one), ("y", one), ("B", 1), ("C", 3), ("H", 12), ("W", 16), ("s", 4), ("xs", 3 * 48 * 64), ("rs", 64), ("dr", 1.0), ("clamp", 1),
        ("eps", 0.0), ("scale", 1.0), ("gx", None), ("loss", one), ("stats", None), ("acc", 0), ("scratch", one), ("stream", None))])
    for bad in (dict(x=None), dict(y=None), dict(loss=None), dict(scratch=None), dict(H=0), dict(W=-3), dict(dr=0.0), dict(dr=float("nan")),
                dict(dr=float("inf")), dict(scale=float("nan")), dict(eps=-1e-3), dict(eps=float("nan")), dict(eps=float("inf")), dict(rs=63),
                dict(xs=3 * 48 * 64 - 3), dict(xs=3 * 48 * 64 + 1), dict(B=0), dict(B=21846), dict(C=2, xs=2 * 48 * 64), dict(s=1), dict(s=5),
                dict(H=4097, xs=3 * 16388 * 64)):
        assert call(**bad) == -2, bad
    assert call(s=5) == -2 and b"2, 3 or 4" in lib.m2t_last_error_string()
    assert call(C=2, xs=2 * 48 * 64) == -2 and b"1 or 3" in lib.m2t_last_error_string()
    assert call(eps=-1.0) == -2 and b"eps" in lib.m2t_last_error_string()
    bp = lambda beta, sr=one, lr=one, sc=one: lib.m2t_back_project_f32(sr, lr, 1, 3, 12, 16, 4, 1.0, beta, 1, None, sc, None)
    for beta in (0.0, 2.0, -1.0, 2.5, float("nan"), float("inf")):
        assert bp(beta) == -2 and b"beta" in lib.m2t_last_error_string(), beta
    assert bp(1.0, sr=None) == -2 and bp(1.0, lr=None) == -2 and bp(1.0, sc=None) == -2
    assert lib.m2t_imresize_adjoint_f32(one, 0, 4, 4, one, 2, 0, None) == -2 and lib.m2t_imresize_adjoint_f32(one, 1, 4, 4, one, 5, 0, None) == -2
    assert lib.m2t_imresize_adjoint_f32(one, 1, 4, 8193, one, 2, 0, None) == -2 and lib.m2t_imresize_adjoint_f32(None, 1, 4, 4, one, 2, 0, None) == -2
    assert lib.m2t_consistency_loss(None, None, 1.0, 1.0, 1.0, 0.0, None, 0, None, None, None) == -2
    assert b"m2t_consistency_loss" in lib.m2t_last_error_string()


def test_python_entries_refuse_host_tensors_and_bad_arguments():
    from m2trans_amd import infer, metrics, resize
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import ConsistencyLoss, consistency_loss
    sr, lr = torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 4, 4)
    for fn in (lambda: consistency_loss(sr, lr, 2), lambda: ConsistencyLoss(2)(sr, lr), lambda: metrics.lr_psnr_device(sr, lr, 2),
               lambda: infer.back_project(sr, lr, 2)):
        with pytest.raises(M2TError, match="device"):
            fn()                                                     # host tensors: no fallback
    with pytest.raises(M2TError, match="device"):
        resize.imresize_adjoint(lr, 2)
    fake = lambda shape, grad=False: types.SimpleNamespace(dim=lambda: 4, shape=torch.Size(shape), is_cuda=True, requires_grad=grad)
    with pytest.raises(M2TError, match="scale must be 2, 3 or 4"):
        consistency_loss(fake((1, 3, 8, 8)), fake((1, 3, 4, 4)), 5)
    with pytest.raises(M2TError, match="expected sr"):
        consistency_loss(fake((1, 3, 8, 9)), fake((1, 3, 4, 4)), 2)
    with pytest.raises(M2TError, match="1 or 3 channels"):
        consistency_loss(fake((1, 2, 8, 8)), fake((1, 2, 4, 4)), 2)
    with pytest.raises(M2TError, match="sr only"):
        consistency_loss(fake((1, 3, 8, 8)), fake((1, 3, 4, 4), True), 2)
    for kw in (dict(eps=-1.0), dict(eps=float("nan")), dict(data_range=0.0), dict(data_range=float("inf"))):
        with pytest.raises(M2TError, match="finite number"):
            consistency_loss(fake((1, 3, 8, 8)), fake((1, 3, 4, 4)), 2, **kw)
    for beta in (0.0, 2.0, float("nan")):
        with pytest.raises(M2TError, match=r"inside \(0, 2\)"):
            infer.back_project(fake((1, 3, 8, 8)), fake((1, 3, 4, 4)), 2, beta=beta)
    with pytest.raises(M2TError, match="iters"):
        infer.back_project(fake((1, 3, 8, 8)), fake((1, 3, 4, 4)), 2, iters=-1)
    with pytest.raises(M2TError):
        ConsistencyLoss(5)
    c = ConsistencyLoss(4, 1e-3, 255.0)
    assert (c.scale, c.eps, c.data_range) == (4, 1e-3, 255.0)
    assert list(inspect.signature(consistency_loss).parameters) == ["sr", "lr", "scale", "eps", "data_range", "clamp"]
    assert list(inspect.signature(infer.back_project).parameters) == ["sr", "lr", "scale", "iters", "beta", "rgb_range", "with_stats"]
    assert inspect.signature(infer.back_project).parameters["iters"].default == 3


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("s", CR.SCALES)
def test_restatement_D_is_imresize_and_the_adjoint_satisfies_the_dot_product_identity(s):
    rng = np.random.default_rng(s)
    for h, w in CR.LR_SHAPES:
        x = rng.standard_normal((2, h * s, w * s))
        g = rng.standard_normal((2, h, w))
        d = CR.down(x, s)
        want = IR.imresize(x, s, False, axes=(1, 2))
        assert np.abs(d - want).max() <= 1e-14 * max(1.0, np.abs(want).max()), (h, w)
        assert np.abs(CR.up(g, s) - IR.imresize(g, s, True, axes=(1, 2))).max() <= 1e-14 * max(1.0, np.abs(g).max())
        lhs, rhs = float((d * g).sum()), float((x * CR.adjoint(g, s)).sum())
        size = float(np.abs(d * g).sum())
        assert abs(lhs - rhs) <= 1e-13 * size, (h, w, lhs, rhs)
        # every row of A sums to 1 (the weights are normalised): D of a constant is that constant, the mirror included
        assert np.abs(CR.A_down(h * s, s).sum(axis=1) - 1.0).max() <= 1e-15


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("s", CR.SCALES)
def test_restatement_gradient_equals_autograd_through_the_dense_matrices(s, clamp):
    h, w, C, R, eps = 5, 7, 3, 1.0, 1e-3
    x, y = CR.loss_case(s, h, w, C)
    scale = 0.37 / y.size
    ref = CR.loss_ref(x, y, s, R, clamp, eps, scale)
    leaf = torch.from_numpy(x).double().requires_grad_(True)
    AH, AW = torch.from_numpy(CR.A_down(h * s, s)), torch.from_numpy(CR.A_down(w * s, s))
    cx = leaf.clamp(0.0, R) if clamp else leaf
    r = (AH @ cx @ AW.T - torch.from_numpy(y).double()) / R
    val = scale * torch.sqrt(r * r + eps * eps).sum()
    val.backward()
    g = leaf.grad.numpy()
    assert abs(float(val.detach()) - ref["value"]) <= 1e-13 * ref["value"]
    # (torch's clamp passes the gradient at the ends of the range, as the definition does)
    assert np.abs(g - ref["grad"]).max() <= 1e-13 * np.abs(ref["grad"]).max()
    if clamp:
        assert np.count_nonzero(ref["grad"][(x < 0) | (x > R)]) == 0 and np.count_nonzero(ref["grad"][(x == 0) | (x == R)]) > 0
    # eps = 0: sign(r), and sign(0) = 0 on the all-black pair
    z = CR.loss_ref(np.zeros_like(x), np.zeros_like(y), s, R, True, 0.0, scale)
    assert z["value"] == 0.0 and np.count_nonzero(z["grad"]) == 0 and z["stats"].tolist() == [0.0, 0.0, 0.0]


def test_back_projection_contracts_for_every_beta_in_0_2():
    """The eigenvalues of A_down A_up per axis are real and inside (0, 1], so 1 - beta * (their products) lies inside (-1, 1) for
    0 < beta < 2: s = 2, 3, 4 and n = s .. 24 s."""
    lo, hi = 1.0, 0.0
    for s in CR.SCALES:
        for m in range(1, 25):
            ev = np.linalg.eigvals(CR.A_down(m * s, s) @ CR.A_up(m, s))
            assert np.abs(ev.imag).max() <= 1e-12, (s, m)
            lo, hi = min(lo, float(ev.real.min())), max(hi, float(ev.real.max()))
            one_minus = 1.0 - ev.real
            assert one_minus.min() > -1.0 and one_minus.max() < 1.0, (s, m)
    print(f"eigenvalues of A_down A_up over s = 2, 3, 4 and n = s .. 24 s: [{lo:.4f}, {hi:.4f}]")
    assert 0.47 <= lo and hi <= 1.0 + 1e-12
    for beta in (0.01, 0.5, 1.0, 1.5, 1.99):                         # 2-D: products of two axis eigenvalues, in [lo^2, 1]
        assert abs(1.0 - beta * lo * lo) < 1.0 and abs(1.0 - beta * hi * hi) < 1.0


@pytest.mark.parametrize("case", CR.BP_MONOTONE, ids=[f"x{c[0]}-{c[1]}x{c[2]}" for c in CR.BP_MONOTONE])
def test_residual_maximum_falls_at_every_iteration_for_the_gpu_tests_inputs(case):
    s, h, w, C, clamp_active = case
    sr0, lr = CR.bp_case(s, h, w, C, clamp_active=clamp_active)
    rows, _ = CR.bp_run(sr0, lr, s, 4, 1.0)
    mx = rows[:, 1].tolist()
    print(f"x{s} {h}x{w}: max |r| over four iterations at beta = 1: {mx}")
    assert all(b < a for a, b in zip(mx, mx[1:])), mx


def test_the_eps_0_inputs_of_the_gpu_test_keep_every_residual_away_from_zero():
    for s in CR.SCALES:
        for h, w in CR.LR_SHAPES:
            for Cn in (1, 3):
                x, y = CR.loss_case(s, h, w, Cn)
                assert CR.loss_ref(x, y, s)["min_abs_r"] >= 1e-9, (s, h, w, Cn)
                assert (x == 0).any() and (x == 1).any()


# ------------------------------------------------------------------------------------------------------------- TrainStep
def test_lambda_consistency_default_resolver_and_setter():
    from m2trans_amd import train_step as T
    from m2trans_amd._lib import M2TError
    sig = inspect.signature(T.TrainStep.__init__).parameters
    assert sig["lambda_consistency"].default == 0.0 and sig["consistency_eps"].default == 0.0
    assert T.TrainStep.lambda_consistency == 0.0 and T.TrainStep.consistency_loss is None and T.TrainStep.consistency_eps == 0.0
    assert T.resolve_lambda_consistency(0) == 0.0 and T.resolve_lambda_consistency("0.5") == 0.5
    for bad in (-0.1, float("nan"), float("inf"), None, "much"):
        with pytest.raises(M2TError, match="lambda_consistency"):
            T.resolve_lambda_consistency(bad)
        with pytest.raises(M2TError, match="consistency_eps"):
            T.resolve_consistency_eps(bad)
    with pytest.raises(M2TError, match="lambda_consistency"):
        T.TrainStep(None, lambda_consistency=-1.0)
    # the last row of the one table: held against the LR image, which sizes its count and its scratch; the scratch entry has a name of
    # its own and takes the scale behind the shape
    row = T._TERM["consistency"]
    assert isinstance(row, T.LossTerm) and T.LOSS_TERMS[-1] is row and row.target == "lr_img"
    assert [t.target for t in T.LOSS_TERMS[:-1]] == ["hr_img"] * 6 and all(t.scratch_entry is None for t in T.LOSS_TERMS[:-1])
    assert row.count(2, 96, 96) == 2 * 3 * 96 * 96 and row.size_ok(1, 1) and row.shape_args(None) == ()
    assert row.scratch_entry == "m2t_consistency_scratch_bytes"
    stand_in = types.SimpleNamespace(model=types.SimpleNamespace(scale=3), consistency_eps=1e-3)
    assert row.scratch_tail(stand_in) == (3,) and row.extra(stand_in) == (1e-3,)
    none = T.TrainStep.__new__(T.TrainStep)
    none.model = stand_in.model
    with pytest.raises(M2TError, match=r"lambda_consistency > 0: no scratch size for a batch of 2 LR images 8x9 at scale 3 \(B \* 3 <= 65535, "
                                       r"SR sides at most 16384\)"):
        none._scratch_for(row, types.SimpleNamespace(m2t_consistency_scratch_bytes=lambda *a: 0), torch.zeros(2, 3, 8, 9))
    ts = T.TrainStep.__new__(T.TrainStep)
    ts.accum_steps, ts.micro_count = 2, 1
    with pytest.raises(M2TError, match="accumulation cycle"):
        ts.set_lambda_consistency(0.0)
    ts.micro_count = 0
    ts.set_lambda_consistency(0.0, 1e-3)
    assert ts.lambda_consistency == 0.0 and ts.consistency_eps == 1e-3 and ts.consistency_loss is None and ts._consistency_scratch == {}
    with pytest.raises(M2TError, match="consistency_eps"):
        ts.set_lambda_consistency(0.0, -1.0)
    assert ts.consistency_eps == 1e-3


class _Calls:
    """A stand-in for the loaded library: records the entry points in call order, every call succeeds."""

    def __init__(self):
        self.names, self.args = [], {}

    def __getattr__(self, name):
        def fn(*a):
            self.names.append(name)
            self.args[name] = a
            return 1 << 20 if name.endswith("scratch_bytes") or name.endswith("workspace_bytes") else 0
        return fn


def _host_step(monkeypatch, accum=1, **terms):
    """TrainStep.forward_backward on the host against _Calls: the step object assembled without __init__, no device needed."""
    from m2trans_amd import _lib, train_step as T
    calls = _Calls()
    monkeypatch.setattr(_lib, "load", lambda: calls)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(_lib, "ptr", lambda t: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    plan = types.SimpleNamespace(handle=None, workspace=None, gen=0, trained=False)
    model = types.SimpleNamespace(scale=2, rgb_range=1.0, flat_params=torch.zeros(4), _plan_for=lambda lr: plan)
    ts = T.TrainStep.__new__(T.TrainStep)
    ts.model, ts.micro_count, ts.accum_steps, ts.world_size = model, 0, accum, 1
    ts.semantic_loss, ts.lambda_clip, ts.lambda_l1 = None, 0.0, 1.0
    ts.grads, ts.micro_grads, ts.l1_loss, ts.micro_loss = torch.zeros(4), torch.zeros(4), torch.zeros(1), torch.zeros(1)
    ts.set_pixel_loss("l1", None)
    for k, v in terms.items():
        if k == "lambda_perceptual":
            ts.perceptual_loss = types.SimpleNamespace(loaded=True, resize=False, data_range=1.0, handle=None, kind=0, param=0.0,
                                                       tap_weights=lambda: None, workspace=lambda *a: None)
            ts.set_lambda_perceptual(v)
        elif k == "lambda_consistency":
            ts.set_lambda_consistency(*v) if isinstance(v, tuple) else ts.set_lambda_consistency(v)
        else:
            getattr(ts, "set_" + k)(v)
    ts.forward_backward(torch.zeros(2, 3, 96, 96), torch.zeros(2, 3, 192, 192))
    return ts, calls


def test_lambda_consistency_zero_issues_todays_call_sequence(monkeypatch):
    today = ["m2t_forward", "m2t_l1_loss_deferred", "m2t_backward"]
    _, bare = _host_step(monkeypatch)
    ts, zero = _host_step(monkeypatch, lambda_consistency=(0.0, 1e-3))
    assert bare.names == today and zero.names == today
    assert ts.consistency_loss is None and ts._consistency_scratch == {}                   # nothing allocated


def test_lambda_consistency_call_sequence_order_divisor_and_accumulation(monkeypatch):
    ts, on = _host_step(monkeypatch, lambda_consistency=(0.05, 1e-3))
    assert on.names == ["m2t_consistency_scratch_bytes", "m2t_forward", "m2t_l1_loss", "m2t_consistency_loss", "m2t_backward"]
    assert on.args["m2t_consistency_scratch_bytes"] == (2, 3, 96, 96, 2)                    # sized by the LR batch and the scale
    a = on.args["m2t_consistency_loss"]
    # weight, divisor = the number of LR elements, R, eps, store
    assert len(a) == 11 and a[2] == 0.05 and a[3] == 2.0 * 3 * 96 * 96 and a[4] == 1.0 and a[5] == 1e-3 and a[7] == 0
    assert list(ts._consistency_scratch) == [(2, 96, 96)] and ts.consistency_loss is not None and ts.loss is not ts.l1_loss
    # pixel -> SSIM -> MS-SSIM -> FFT -> VIF -> GMSD -> wavelet -> consistency -> perceptual -> backward
    _, every = _host_step(monkeypatch, lambda_ssim=0.1, lambda_msssim=0.16, lambda_fft=0.1, lambda_vif=0.05, lambda_gmsd=0.05,
                          lambda_wavelet=0.1, lambda_consistency=0.05, lambda_perceptual=0.2)
    order = [n for n in every.names if not n.endswith("scratch_bytes")]
    assert order == ["m2t_forward", "m2t_l1_loss", "m2t_ssim_loss", "m2t_msssim_loss", "m2t_fft_loss", "m2t_vif_loss", "m2t_gmsd_loss",
                     "m2t_wavelet_loss", "m2t_consistency_loss", "m2t_vgg_loss", "m2t_backward"]
    # the second micro-batch of a cycle: the divisor is the global number of LR elements, the value is added to
    ts, acc = _host_step(monkeypatch, accum=2, lambda_consistency=0.05)
    assert acc.args["m2t_consistency_loss"][3] == 2 * 2.0 * 3 * 96 * 96 and acc.args["m2t_consistency_loss"][7] == 0
    ts.forward_backward(torch.zeros(2, 3, 96, 96), torch.zeros(2, 3, 192, 192))
    assert acc.args["m2t_consistency_loss"][7] == 1 and acc.names.count("m2t_consistency_scratch_bytes") == 1


def test_meter_columns_and_the_train_keys():
    from m2trans_amd import train as TR
    assert "lambda_consistency" in TR.TRAINSTEP_KEYS and "consistency_eps" in TR.TRAINSTEP_KEYS
    off = types.SimpleNamespace(lambda_vif=0.1)
    assert TR.meter_columns(off) == ["loss", "pixel", "clip", "vif"]
    on = types.SimpleNamespace(lambda_wavelet=0.1, lambda_consistency=0.05, lambda_perceptual=0.2, loss=1, l1_loss=2, clip_loss=3,
                               wavelet_loss=4, consistency_loss=5, perceptual_loss_value=6)
    cols = TR.meter_columns(on)
    assert cols == ["loss", "pixel", "clip", "wavelet", "consistency", "perceptual"]
    assert TR.meter_values(on, cols) == [1, 2, 3, 4, 5, 6]


def _cfg(**more):
    cfg = {"scale": 4, "patch_size": 64, "batch_size": 2, "epochs": 1, "lr": 1e-4, "eta_min": 1e-6, "log_every": 1, "test_every": 1,
           "training_dataset": "folder", "train_hr_path": "somewhere"}
    cfg.update(more)
    return cfg


def test_train_config_takes_both_keys_and_refuses_them_next_to_a_degradation():
    from m2trans_amd import train as TR
    from m2trans_amd._lib import M2TError
    r = TR.resolve_config(_cfg(lambda_consistency=0.05, consistency_eps=1e-3))
    assert r["train_step"]["lambda_consistency"] == 0.05 and r["train_step"]["consistency_eps"] == 1e-3
    assert "lambda_consistency" not in TR.resolve_config(_cfg())["train_step"]
    deg = {"bank": 16, "noise": [0, 5], "gray_noise": False}
    assert TR.resolve_config(_cfg(degradation=deg))["data"]["degradation"] == deg
    with pytest.raises(M2TError, match=r"lambda_consistency.*degradation"):
        TR.resolve_config(_cfg(degradation=deg, lambda_consistency=0.05))
    assert TR.resolve_config(_cfg(degradation=deg, lambda_consistency=0.0))["data"]["degradation"] is not None


# ------------------------------------------------------------------------------------------------------------- checkpoint
def _model():
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))


class _Step:
    """The flat-buffer part of TrainStep on the CPU, with the pixel loss and the weights of the optional terms."""

    def __init__(self, m, step_count=7, lr=5e-5, consistency_eps=0.0, **lambdas):
        from m2trans_amd.train_step import TrainStep
        g = torch.Generator().manual_seed(step_count)
        self.exp_avg = torch.randn(m.flat_params.shape, generator=g)
        self.exp_avg_sq = torch.rand(m.flat_params.shape, generator=g)
        self.step_count, self.lr, self.scheduler_last_epoch = step_count, lr, 0
        self.micro_count, self.accum_steps, self.fft_norm = 0, 1, "backward"
        TrainStep.set_pixel_loss(self, "l1", None)
        for n in ("ssim", "msssim", "fft", "vif", "gmsd", "wavelet", "consistency"):
            setattr(self, f"lambda_{n}", float(lambdas.get(f"lambda_{n}", 0.0)))
        self.consistency_eps = consistency_eps

    def set_pixel_loss(self, name, param=None):
        from m2trans_amd.train_step import TrainStep
        TrainStep.set_pixel_loss(self, name, param)

    def set_lambda_consistency(self, value, eps=None):
        from m2trans_amd.train_step import resolve_consistency_eps, resolve_lambda_consistency
        self.lambda_consistency = resolve_lambda_consistency(value)
        if eps is not None:
            self.consistency_eps = resolve_consistency_eps(eps)

    def set_lr(self, lr):
        self.lr = lr


def test_checkpoint_entry_carries_both_keys_after_the_existing_ones_and_round_trips():
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model()
    keys = ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict"]
    assert list(export_checkpoint(m, _Step(m, lambda_consistency=0.0, consistency_eps=1e-3), epoch=3)) == keys      # off: today's dict
    src = _Step(m, lambda_consistency=0.05, consistency_eps=1e-3)
    ck = export_checkpoint(m, src, epoch=3)
    assert list(ck) == keys + ["m2t_loss"]
    assert ck["m2t_loss"] == {"pixel_loss": "l1", "param": None, "lambda_consistency": 0.05, "consistency_eps": 1e-3}
    both = export_checkpoint(m, _Step(m, lambda_consistency=0.05, lambda_ssim=0.1, lambda_gmsd=0.2), epoch=3)["m2t_loss"]
    assert list(both) == ["pixel_loss", "param", "lambda_ssim", "lambda_gmsd", "lambda_consistency", "consistency_eps"]
    for start in (0.0, 0.7):
        dst = _Step(_model(), lambda_consistency=start, step_count=1)
        assert import_checkpoint(ck, _model(), dst) == 4
        assert dst.lambda_consistency == 0.05 and dst.consistency_eps == 1e-3 and dst.step_count == 7 and torch.equal(dst.exp_avg, src.exp_avg)
    # a file without the key leaves a fresh step at 0
    dst = _Step(_model())
    import_checkpoint(export_checkpoint(m, _Step(m, lambda_gmsd=0.3), epoch=3), _model(), dst)
    assert dst.lambda_consistency == 0.0
    # a plain object without the setters receives the attributes
    plain = types.SimpleNamespace(lr=1.0, step_count=0, exp_avg=torch.zeros_like(m.flat_params), exp_avg_sq=torch.zeros_like(m.flat_params),
                                  scheduler_last_epoch=0, set_lr=lambda lr: None)
    import_checkpoint(ck, _model(), plain)
    assert plain.lambda_consistency == 0.05 and plain.consistency_eps == 1e-3


# ------------------------------------------------------------------------------------------------------------- command line
def test_command_line_parses_back_project_and_its_step():
    from m2trans_amd import infer
    base = ["--config", "c", "--model_path", "m", "--input", "i", "--output", "o"]
    a = infer.parse_args(base)
    assert a.back_project is None and a.back_project_beta is None
    a = infer.parse_args(base + ["--back_project", "3"])
    assert a.back_project == 3 and a.back_project_beta == 1.0
    a = infer.parse_args(base + ["--back_project", "2", "--back_project_beta", "0.5", "--tile", "64", "--self_ensemble"])
    assert a.back_project == 2 and a.back_project_beta == 0.5 and a.tile == 64
    for bad in (["--back_project", "0"], ["--back_project_beta", "1.0"], ["--back_project", "2", "--back_project_beta", "2.0"],
                ["--back_project", "2", "--back_project_beta", "0"]):
        with pytest.raises(SystemExit):
            infer.parse_args(base + bad)
    kw = inspect.signature(infer.upscale_folder).parameters
    assert kw["back_project_iters"].default == 0 and kw["back_project_beta"].default == 1.0
    rec = infer.consistency_record(torch.tensor([[0.1, 0.5, 1e-2], [0.05, 0.2, 1e-3], [0.0, 0.0, 0.0]], dtype=torch.float64))
    assert rec["before"] == {"mean_residual": 0.1, "max_residual": 0.5, "lr_psnr": 20.0} and rec["after"]["lr_psnr"] == float("inf")
    assert inspect.signature(infer.BackProject.__init__).parameters["iters"].default == 3


def test_timing_tool_builds_its_json_line_from_the_repeat_times():
    import importlib.util
    spec = importlib.util.spec_from_file_location("consistency_timing", os.path.join(ROOT, "tools", "consistency_timing.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse_args([])
    assert (args.batch, args.lr_size, args.blocks, args.dtype) == (16, 128, 8, "bf16")            # configs[1]
    with pytest.raises(SystemExit):
        tool.parse_args(["--repeats", "2"])
    mb = tool.traffic_mb(16, 128)
    # forward: 50.3 MB of SR and 3.1 MB of LR read, 6.3 MB of fp64 plane written; the seed's read-modify-write is 100.7 MB
    assert mb["forward"] == 59.77 and mb["copy_of_sr"] == 100.66 and mb["backward"] == 157.29
    ms = {"l1": [4.0, 4.2, 4.1], "l1+consistency": [4.3, 4.2, 4.4], "l1+ssim": [5.0, 5.1, 5.2]}
    kms = {k: [0.1, 0.3, 0.2] for k in tool.KERNELS}
    out = tool.result(args, ms, kms)
    assert tuple(out) == tool.RESULT_KEYS and out["ms_per_step"] == {"l1": 4.1, "l1+consistency": 4.3, "l1+ssim": 5.1}
    assert out["l1_spread"] == round(0.2 / 4.1, 4) and out["added_ms"]["l1+consistency"] == 0.2 and out["kernels_ms"]["term"] == 0.2
    assert out["implied_ms_at_6_3_tb_s"]["copy_of_sr"] == round(100.66 / 6300.0, 4)


# ------------------------------------------------------------------------------------------------------------- host emulation
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    import subprocess
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"), shutil.which("clang++"), shutil.which("g++"))
                if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("consistency") / "consistency_emulate")
    subprocess.run([cxx, "-x", "c++", "-std=c++20", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "emulate_hip"),
                    "-I", os.path.join(ROOT, "m2trans_amd", "csrc"), os.path.join(ROOT, "tests", "consistency_emulate.cpp"), "-o", exe, "-lpthread"],
                   check=True, capture_output=True)
    return exe


def _emulate(exe, tmp_path, mode, s, h, w, rs, planes, clamp, acc, R, eps, scale, x, y, gx):
    import subprocess
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("8i", mode, s, h, w, rs, planes, clamp, acc) + struct.pack("f", R) + struct.pack("2d", eps, scale))
        f.write(np.ascontiguousarray(x, dtype=np.float32).tobytes() + np.ascontiguousarray(y, dtype=np.float32).tobytes()
                + np.ascontiguousarray(gx, dtype=np.float32).tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, capture_output=True)
    b = open(tmp_path / "out.bin", "rb").read()
    return (struct.unpack("f", b[:4])[0], np.frombuffer(b[4:28], dtype=np.float64),
            np.frombuffer(b[28:], dtype=np.float32).reshape(planes, h * s, rs))


def _ratio(got, ref, gate):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    ratio = np.where(gate > 0, err / np.maximum(gate, 1e-300), np.where(err > 0, np.inf, 0.0))
    return int((err > gate).sum()), float(ratio.max())


EMU_SHAPES = [(1, 1), (2, 3), (5, 7), (16, 32), (17, 33)]


@pytest.mark.parametrize("eps", [0.0, 1e-3])
@pytest.mark.parametrize("s", CR.SCALES)
def test_loss_kernel_text_emulated_on_the_host_meets_the_gpu_gate(emulator, tmp_path, s, eps):
    """csrc/m2t_consistency_tile.h -- the text the kernels run -- on host threads, the kernels' own sum order, from a NaN-filled
    scratch: x in a NaN-filled buffer with a longer row; the gradient within the gate of the GPU test, the value within fp32 rounding,
    the statistics at 1e-12, exact zeros under the clamp, nothing written outside [Hs, Ws], accumulate on the value."""
    for h, w in EMU_SHAPES:
        for Cn in (1, 3):
            x, y = CR.loss_case(s, h, w, Cn)
            planes, Hs, Ws, rs = x.shape[0] * Cn, h * s, w * s, w * s + 3
            scale = 0.37 / y.size
            ref = CR.loss_ref(x, y, s, 1.0, True, eps, scale)
            xb = np.full((planes, Hs, rs), np.nan, np.float32)
            xb[:, :, :Ws] = x.reshape(planes, Hs, Ws)
            seed = np.zeros_like(xb)
            seed[:, :, Ws:] = np.nan
            loss, stats, gx = _emulate(emulator, tmp_path, 0, s, h, w, rs, planes, 1, 1, 1.0, eps, scale, xb, y, seed)
            got = gx[:, :, :Ws].reshape(x.shape)
            nbad, worst = _ratio(got, ref["grad"], ref["gate"])
            assert nbad == 0, f"x{s} {h}x{w} C{Cn}: {nbad} elements beyond the gate, worst ratio {worst:.3f}"
            assert np.isnan(gx[:, :, Ws:]).all() and np.count_nonzero(got[ref["mask"] == 0]) == 0
            assert abs(loss - 0.25 - ref["value"]) <= 1.2e-7 * (0.25 + ref["value"])                    # (the emulator starts the value at 0.25)
            assert np.all(np.abs(stats - ref["stats"]) <= 1e-12 * ref["stats"])


@pytest.mark.parametrize("s", CR.SCALES)
def test_adjoint_kernel_text_emulated_on_the_host_meets_the_gpu_gate(emulator, tmp_path, s):
    rng = np.random.default_rng(50 + s)
    for h, w in EMU_SHAPES + [(3, 40)]:
        g = rng.standard_normal((2, h, w)).astype(np.float32)
        ref = CR.adjoint(g, s)
        gate = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * CR.adjoint_abs(g, s)
        nanout = np.full((2, h * s, w * s), np.nan, np.float32)
        _, _, out = _emulate(emulator, tmp_path, 2, s, h, w, w * s, 2, 0, 0, 1.0, 0.0, 1.0, np.zeros_like(nanout), g, nanout)
        nbad, worst = _ratio(out, ref, gate)
        assert nbad == 0, (s, h, w, nbad, worst)
        half = np.full_like(nanout, 0.5)
        _, _, acc = _emulate(emulator, tmp_path, 2, s, h, w, w * s, 2, 0, 1, 1.0, 0.0, 1.0, np.zeros_like(nanout), g, half)
        assert np.array_equal(acc, half + out)


@pytest.mark.parametrize("case", CR.BP_CASES, ids=[f"x{c[0]}-{c[1]}x{c[2]}" for c in CR.BP_CASES])
def test_back_projection_kernel_text_emulated_on_the_host_meets_the_gpu_gate(emulator, tmp_path, case):
    s, h, w, Cn, clamp_active = case
    sr0, lr = CR.bp_case(s, h, w, Cn, clamp_active=clamp_active)
    planes = sr0.shape[0] * Cn
    for beta in (0.5, 1.5):
        cur = sr0.copy()
        for it in range(2):
            ref = CR.back_project_ref(cur, lr, s, 1.0, beta)
            _, stats, new = _emulate(emulator, tmp_path, 1, s, h, w, w * s, planes, 1, 0, 1.0, 0.0, beta, cur, lr, np.zeros_like(cur))
            new = new.reshape(cur.shape)
            nbad, worst = _ratio(new, ref["new"], ref["gate"])
            assert nbad == 0, (case, beta, it, nbad, worst)
            assert np.all(np.abs(stats - ref["stats"]) <= 1e-12 * ref["stats"])
            assert new.min() >= 0.0 and new.max() <= 1.0
            cur = new.copy()
