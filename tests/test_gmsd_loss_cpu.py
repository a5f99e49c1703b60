"""CPU tests (no GPU) of the GMSD loss term (TrainStep(lambda_gmsd=...), m2t_gmsd_loss / m2t_gmsd_loss_tensor): the fp64 restatement
the GPU tests compare the kernels with (tests/gmsd_loss_ref.py) -- its value against the oracle's gmsd, its closed-form gradient against
torch autograd of that oracle where autograd is finite, the two conventions where it is not -- the C ABI table of include/m2t_gmsd.h,
TrainStep's argument validation and call sequence, the checkpoint entry, the train.py key, and the kernel text run on host threads
(tests/gmsd_emulate.cpp) under the gate of the GPU test."""
import contextlib
import ctypes as C
import inspect
import os
import re
import shutil
import struct
import types

import pytest
import torch

from oracle.m2trans_oracle import gmsd as oracle_gmsd
from tests import gmsd_loss_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_ULP = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------- the restatement
def _noisy(shape, seed, R):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g) * 1.2 - 0.1) * R          # a share outside [0, R]; no flat entry
    y = torch.rand(shape, generator=g) * R
    return x.float(), y.float()


@pytest.mark.parametrize("shape", [(2, 3, 5, 6), (2, 3, 33, 70), (1, 3, 64, 64)], ids=["5x6", "33x70", "64x64"])
@pytest.mark.parametrize("R", [1.0, 255.0])
@pytest.mark.parametrize("clamp", [False, True])
def test_restatement_equals_the_oracle_and_its_autograd_where_nothing_is_flat(shape, R, clamp):
    """Value against oracle.m2trans_oracle.gmsd in fp64, the closed-form gradient against autograd of that oracle: <= 1e-12."""
    x, y = _noisy(shape, 1, R)
    val, grad, gm, shares = G.value_and_grad(x, y, R, clamp)
    assert shares["dead"] == 0.0 and shares["clamped"] > 0
    leaf = x.double().requires_grad_(True)
    o = oracle_gmsd(leaf.clamp(0.0, R) if clamp else leaf, y.double(), R)
    o.mean().backward()
    assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    ev, eg = float((gm - o.detach()).abs().max()), float((grad - leaf.grad).abs().max())
    print(f"{shape} R {R:g} clamp {clamp}: GMSD {gm.tolist()}, value error {ev:.2e}, gradient error {eg:.2e}")
    assert ev <= 1e-12 and eg <= 1e-12 and abs(float(val) - float(o.detach().mean())) <= 1e-12
    if clamp:
        assert int(torch.count_nonzero(grad[(x < 0) | (x > R)])) == 0


def test_autograd_is_nan_on_flat_entries_and_the_restatement_is_finite_and_exactly_zero_there():
    shape = (1, 3, 33, 70)
    x, y = G.mixed_pair(shape, seed=3)
    leaf = x.double().requires_grad_(True)
    oracle_gmsd(leaf, y.double()).mean().backward()
    assert int(torch.isnan(leaf.grad).sum()) > 0                       # 0 * inf from sqrt(0)
    val, grad, gm, shares = G.value_and_grad(x, y, 1.0, True, min_gmsd=1e-3)
    assert min(shares.values()) > 0, shares
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    sec = G.sector(shape)
    assert int(sec.sum()) > 0 and int(torch.count_nonzero(grad[sec])) == 0
    assert abs(float(gm) - float(oracle_gmsd(x.double().clamp(0, 1), y.double()))) <= 1e-12
    # the 16 x 16 pair whose left half is zero: half of autograd's elements are NaN
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(1, 3, 16, 16, generator=g, dtype=torch.float64), torch.rand(1, 3, 16, 16, generator=g, dtype=torch.float64)
    a[..., :8], b[..., :8] = 0.0, 0.0
    leaf = a.clone().requires_grad_(True)
    oracle_gmsd(leaf, b).mean().backward()
    assert int(torch.isnan(leaf.grad).sum()) == 384
    assert bool(torch.isfinite(G.value_and_grad(a, b)[1]).all())


def test_identical_images_and_one_cell_images_give_zero_and_no_gradient():
    x, y = G.mixed_pair((2, 3, 12, 14), seed=4)
    val, grad, gm, _ = G.value_and_grad(y, y)
    assert float(val) == 0.0 and gm.tolist() == [0.0, 0.0] and int(torch.count_nonzero(grad)) == 0
    a, b = torch.rand(1, 3, 2, 2), torch.rand(1, 3, 2, 2)
    val, grad, gm, _ = G.value_and_grad(a, b)
    assert float(val) == 0.0 and float(gm) == 0.0 and int(torch.count_nonzero(grad)) == 0
    # one image of the batch identical: only that image has no gradient
    x[0] = y[0]
    _, grad, gm, _ = G.value_and_grad(x, y)
    assert float(gm[0]) == 0.0 and float(gm[1]) > 0 and int(torch.count_nonzero(grad[0])) == 0 and int(torch.count_nonzero(grad[1])) > 0


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_decide_sizes_and_bad_arguments_on_the_host():
    from m2trans_amd import _lib
    lib = _lib.load()
    sb = lib.m2t_gmsd_loss_scratch_bytes
    assert sb(2, 3, 1, 64) == 0 and sb(2, 3, 64, 1) == 0 and sb(0, 3, 64, 64) == 0 and sb(65536, 3, 64, 64) == 0
    assert sb(1, 2, 64, 64) == 0 and sb(1, 4, 64, 64) == 0
    # the record (4 doubles) and two sums per 32 x 32-cell tile, per image; the channel count changes nothing
    assert sb(1, 1, 2, 2) == sb(1, 3, 2, 2) == 8 * (4 + 2) and sb(1, 3, 64, 64) == 8 * (4 + 2)
    assert sb(2, 3, 33, 70) == 2 * 8 * (4 + 2 * 2) and sb(1, 3, 70, 33) == 8 * (4 + 2 * 2) and sb(1, 1, 64, 130) == 8 * (4 + 2 * 3)
    assert sb(16, 3, 512, 512) == 16 * 8 * (4 + 2 * 64)
    one = C.c_void_p(8)                                              # a non-null pointer that is never followed
    call = lambda **kw: lib.m2t_gmsd_loss_tensor(*[kw.get(k, v) for k, v in (
        ("x", one), ("y", one), ("B", 1), ("C", 3), ("H", 48), ("W", 64), ("xs", 3 * 48 * 64), ("rs", 64), ("dr", 1.0), ("clamp", 1),
        ("scale", 1.0), ("gx", None), ("loss", one), ("per", None), ("acc", 0), ("scratch", one), ("stream", None))])
    for bad in (dict(x=None), dict(y=None), dict(loss=None), dict(scratch=None), dict(H=1), dict(W=1), dict(H=0), dict(W=-3), dict(dr=0.0),
                dict(dr=-1.0), dict(dr=float("nan")), dict(dr=float("inf")), dict(scale=float("nan")), dict(scale=float("inf")),
                dict(rs=63), dict(xs=3 * 48 * 64 - 3), dict(xs=3 * 48 * 64 + 1), dict(B=0), dict(B=-1), dict(B=65536),
                dict(C=0), dict(C=2, xs=2 * 48 * 64), dict(C=4, xs=4 * 48 * 64)):
        assert call(**bad) == -2, bad
    assert call(H=1) == -2 and b"at least 2" in lib.m2t_last_error_string()
    assert call(C=2, xs=2 * 48 * 64) == -2 and b"1 or 3" in lib.m2t_last_error_string()
    assert call(B=65536) == -2 and b"65535" in lib.m2t_last_error_string()
    assert lib.m2t_gmsd_loss(None, None, 1.0, 1.0, 1.0, None, 0, None, None, None) == -2
    assert b"m2t_gmsd_loss" in lib.m2t_last_error_string()


def test_python_entries_refuse_host_tensors_and_bad_arguments():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import GMSDLoss, gmsd_loss
    x = torch.zeros(1, 3, 8, 8)
    for fn in (gmsd_loss, GMSDLoss()):
        with pytest.raises(M2TError, match="device"):
            fn(x, x)                                                 # host tensors: no fallback
        with pytest.raises(M2TError):
            fn(x, x[..., :6])
    fake = types.SimpleNamespace(dim=lambda: 4, shape=torch.Size((1, 3, 8, 8)), is_cuda=True, requires_grad=False)
    for kw in (dict(data_range=0.0), dict(data_range=float("nan")), dict(data_range=float("inf"))):
        with pytest.raises(M2TError, match="finite number > 0"):
            gmsd_loss(fake, fake, **kw)
    two = types.SimpleNamespace(dim=lambda: 4, shape=torch.Size((1, 2, 8, 8)), is_cuda=True, requires_grad=False)
    with pytest.raises(M2TError, match="1 or 3 channels"):
        gmsd_loss(two, two)
    small = types.SimpleNamespace(dim=lambda: 4, shape=torch.Size((1, 3, 1, 8)), is_cuda=True, requires_grad=False)
    with pytest.raises(M2TError, match="at least 2"):
        gmsd_loss(small, small)
    needs = types.SimpleNamespace(dim=lambda: 4, shape=torch.Size((1, 3, 8, 8)), is_cuda=True, requires_grad=True)
    with pytest.raises(M2TError, match="x only"):
        gmsd_loss(fake, needs)
    assert GMSDLoss(255.0).data_range == 255.0


# ------------------------------------------------------------------------------------------------------------- TrainStep
def test_lambda_gmsd_default_resolver_setter_and_table():
    from m2trans_amd import train_step as T
    from m2trans_amd._lib import M2TError
    assert inspect.signature(T.TrainStep.__init__).parameters["lambda_gmsd"].default == 0.0
    assert T.TrainStep.lambda_gmsd == 0.0 and T.TrainStep.gmsd_loss is None
    assert T.resolve_lambda_gmsd(0) == 0.0 and T.resolve_lambda_gmsd(0.05) == 0.05 and T.resolve_lambda_gmsd("0.5") == 0.5
    for bad in (-0.1, float("nan"), float("inf"), None, "much"):
        with pytest.raises(M2TError, match="lambda_gmsd"):
            T.resolve_lambda_gmsd(bad)
    with pytest.raises(M2TError, match="lambda_gmsd"):
        T.TrainStep(None, lambda_gmsd=-1.0)
    # the row of the one table (its order: tests/test_loss_terms_cpu.py)
    row = T._TERM["gmsd"]
    assert isinstance(row, T.LossTerm) and row in T.LOSS_TERMS
    assert row.size_ok(2, 2) and row.size_ok(2, 500) and not row.size_ok(1, 500) and not row.size_ok(500, 1)
    assert row.count(7, 100, 200) == 7 and row.extra(None) == ()
    ts = T.TrainStep.__new__(T.TrainStep)
    ts.accum_steps, ts.micro_count = 2, 1
    with pytest.raises(M2TError, match="accumulation cycle"):
        ts.set_lambda_gmsd(0.0)
    ts.micro_count = 0
    ts.set_lambda_gmsd(0.0)
    assert ts.lambda_gmsd == 0.0 and ts.gmsd_loss is None and ts._gmsd_scratch == {}
    # a size the term does not take is refused on the host: no library call is made (lib = None would raise otherwise)
    with pytest.raises(M2TError, match="lambda_gmsd > 0: .*at least 2"):
        ts._scratch_for(row, None, torch.zeros(2, 3, 1, 64))


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
        else:
            getattr(ts, "set_" + k)(v)
    ts.forward_backward(torch.zeros(2, 3, 96, 96), torch.zeros(2, 3, 192, 192))
    return ts, calls


def test_lambda_gmsd_zero_issues_todays_call_sequence(monkeypatch):
    today = ["m2t_forward", "m2t_l1_loss_deferred", "m2t_backward"]
    _, bare = _host_step(monkeypatch)
    ts, zero = _host_step(monkeypatch, lambda_gmsd=0.0)
    assert bare.names == today and zero.names == today
    assert ts.gmsd_loss is None and ts._gmsd_scratch == {}              # nothing allocated


def test_lambda_gmsd_call_sequence_alone_and_with_vif_and_perceptual(monkeypatch):
    ts, on = _host_step(monkeypatch, lambda_gmsd=0.05)
    assert on.names == ["m2t_gmsd_loss_scratch_bytes", "m2t_forward", "m2t_l1_loss", "m2t_gmsd_loss", "m2t_backward"]
    assert on.args["m2t_gmsd_loss_scratch_bytes"] == (2, 3, 192, 192)
    a = on.args["m2t_gmsd_loss"]
    assert len(a) == 10 and a[2] == 0.05 and a[3] == 2.0 and a[4] == 1.0 and a[6] == 0     # weight, divisor = B, R, store
    assert list(ts._gmsd_scratch) == [(2, 192, 192)] and ts.gmsd_loss is not None
    assert ts.loss is not ts.l1_loss
    ts, both = _host_step(monkeypatch, lambda_vif=0.1, lambda_gmsd=0.05, lambda_perceptual=0.2)
    order = [n for n in both.names if not n.endswith("scratch_bytes")]
    assert order == ["m2t_forward", "m2t_l1_loss", "m2t_vif_loss", "m2t_gmsd_loss", "m2t_vgg_loss", "m2t_backward"]
    _, every = _host_step(monkeypatch, lambda_ssim=0.1, lambda_msssim=0.16, lambda_fft=0.1, lambda_vif=0.05, lambda_gmsd=0.05)
    order = [n for n in every.names if not n.endswith("scratch_bytes")]
    assert order == ["m2t_forward", "m2t_l1_loss", "m2t_ssim_loss", "m2t_msssim_loss", "m2t_fft_loss", "m2t_vif_loss", "m2t_gmsd_loss",
                     "m2t_backward"]
    # the second micro-batch of a cycle: the divisor is the global number of images, the value is added to
    ts, acc = _host_step(monkeypatch, accum=2, lambda_gmsd=0.05)
    assert acc.args["m2t_gmsd_loss"][3] == 4.0 and acc.args["m2t_gmsd_loss"][6] == 0
    ts.forward_backward(torch.zeros(2, 3, 96, 96), torch.zeros(2, 3, 192, 192))
    assert acc.args["m2t_gmsd_loss"][6] == 1 and acc.names.count("m2t_gmsd_loss_scratch_bytes") == 1


def test_meter_columns_and_the_train_key():
    from m2trans_amd import train as TR
    assert "lambda_gmsd" in TR.TRAINSTEP_KEYS and TR.TRAINSTEP_KEYS.index("lambda_gmsd") == TR.TRAINSTEP_KEYS.index("lambda_vif") + 1
    off = types.SimpleNamespace(lambda_vif=0.1)
    assert TR.meter_columns(off) == ["loss", "pixel", "clip", "vif"]
    on = types.SimpleNamespace(lambda_vif=0.1, lambda_gmsd=0.05, lambda_perceptual=0.2, loss=1, l1_loss=2, clip_loss=3, vif_loss=4, gmsd_loss=5,
                               perceptual_loss_value=6)
    cols = TR.meter_columns(on)
    assert cols == ["loss", "pixel", "clip", "vif", "gmsd", "perceptual"]
    assert TR.meter_values(on, cols) == [1, 2, 3, 4, 5, 6]


# ------------------------------------------------------------------------------------------------------------- checkpoint
def _model():
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))


class _Step:
    """The flat-buffer part of TrainStep on the CPU, with the pixel loss and the weights of the optional terms."""

    def __init__(self, m, pixel_loss="l1", pixel_loss_param=None, step_count=7, lr=5e-5, **lambdas):
        from m2trans_amd.train_step import TrainStep
        g = torch.Generator().manual_seed(step_count)
        self.exp_avg = torch.randn(m.flat_params.shape, generator=g)
        self.exp_avg_sq = torch.rand(m.flat_params.shape, generator=g)
        self.step_count, self.lr, self.scheduler_last_epoch = step_count, lr, 0
        self.micro_count, self.accum_steps, self.fft_norm = 0, 1, "backward"
        TrainStep.set_pixel_loss(self, pixel_loss, pixel_loss_param)
        for n in ("ssim", "msssim", "fft", "vif", "gmsd"):
            setattr(self, f"lambda_{n}", float(lambdas.get(f"lambda_{n}", 0.0)))

    def set_pixel_loss(self, name, param=None):
        from m2trans_amd.train_step import TrainStep
        TrainStep.set_pixel_loss(self, name, param)

    def set_lambda_gmsd(self, value):
        from m2trans_amd.train_step import resolve_lambda_gmsd
        self.lambda_gmsd = resolve_lambda_gmsd(value)

    def set_lr(self, lr):
        self.lr = lr


def test_checkpoint_entry_carries_lambda_gmsd_after_the_existing_keys_and_round_trips():
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model()
    keys = ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict"]
    assert list(export_checkpoint(m, _Step(m, lambda_gmsd=0.0), epoch=3)) == keys           # off: today's dict
    src = _Step(m, "sl1", 0.25, lambda_gmsd=0.05)
    ck = export_checkpoint(m, src, epoch=3)
    assert list(ck) == keys + ["m2t_loss"]
    assert ck["m2t_loss"] == {"pixel_loss": "smooth_l1", "param": 0.25, "lambda_gmsd": 0.05}
    every = export_checkpoint(m, _Step(m, lambda_gmsd=0.05, lambda_ssim=0.1, lambda_msssim=0.16, lambda_fft=0.2, lambda_vif=0.3), epoch=3)["m2t_loss"]
    assert list(every) == ["pixel_loss", "param", "lambda_ssim", "lambda_msssim", "lambda_fft", "fft_norm", "lambda_vif", "lambda_gmsd"]
    for start in (0.0, 0.7):                                                      # whatever the importing step was built with
        dst = _Step(_model(), "mse", None, lambda_gmsd=start, step_count=1)
        assert import_checkpoint(ck, _model(), dst) == 4
        assert dst.lambda_gmsd == 0.05 and (dst.pixel_loss, dst.pixel_loss_param) == ("smooth_l1", 0.25)
        assert dst.step_count == 7 and torch.equal(dst.exp_avg, src.exp_avg)
    # a file without the key loads as 0 into a fresh step
    dst = _Step(_model())
    import_checkpoint(export_checkpoint(m, _Step(m, "mse", lambda_vif=0.3), epoch=3), _model(), dst)
    assert dst.lambda_gmsd == 0.0 and dst.pixel_loss == "mse"
    import_checkpoint(export_checkpoint(m, _Step(m), epoch=3), _model(), dst)
    assert dst.lambda_gmsd == 0.0
    # a plain object without the setters receives the attribute
    plain = types.SimpleNamespace(lr=1.0, step_count=0, exp_avg=torch.zeros_like(m.flat_params), exp_avg_sq=torch.zeros_like(m.flat_params),
                                  scheduler_last_epoch=0, set_lr=lambda lr: None)
    import_checkpoint(ck, _model(), plain)
    assert plain.lambda_gmsd == 0.05


# ------------------------------------------------------------------------------------------------------------- host emulation
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    import subprocess
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"), shutil.which("clang++"), shutil.which("g++"))
                if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("gmsd") / "gmsd_emulate")
    subprocess.run([cxx, "-x", "c++", "-std=c++20", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "emulate_hip"),
                    "-I", os.path.join(ROOT, "m2trans_amd", "csrc"), os.path.join(ROOT, "tests", "gmsd_emulate.cpp"), "-o", exe, "-lpthread"],
                   check=True, capture_output=True)
    return exe


def gate(got, ref, prefill=None):
    """(elements beyond the gate of the GPU test, largest |got - want| / bound): 1e-6 |ref| + 1e-7 max |ref| + 2^-24 |want|."""
    top = ref.abs().amax(dim=(-3, -2, -1), keepdim=True)
    want = ref if prefill is None else prefill + ref
    bound = 1e-6 * ref.abs() + 1e-7 * top + HALF_ULP * want.abs()
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return int((err > bound).sum()), float(ratio.max())


@pytest.mark.parametrize("H,W,rs,Cn,Rr,clamp,vec", [(5, 6, 6, 3, 1.0, 1, 1), (33, 70, 80, 3, 255.0, 1, 1), (70, 33, 33, 3, 1.0, 0, 1),
                                                   (64, 130, 132, 1, 1.0, 1, 1), (64, 130, 130, 1, 255.0, 1, 0), (2, 2, 2, 3, 1.0, 1, 1)],
                         ids=["5x6", "33x70-stride80", "70x33", "64x130-vec", "64x130-scalar", "2x2"])
def test_kernel_text_emulated_on_the_host_meets_the_gpu_gate(emulator, tmp_path, H, W, rs, Cn, Rr, clamp, vec):
    """csrc/m2t_gmsd_tile.h -- the text the kernels run -- on host threads (tests/gmsd_emulate.cpp), the kernel's own sum order: every
    shape of the GPU test, the 16-byte path and the scalar one, x in a NaN-filled buffer with a longer row.  The gradient within the
    gate of the GPU test, GMSD within 1e-12, the value within fp32 rounding, exact zeros on the sector and under the clamp, nothing
    written outside [H, W]."""
    import subprocess
    import numpy as np
    scale = 0.37
    shape = (1, Cn, H, W)
    x, y = G.mixed_pair(shape, seed=12, R=Rr)
    want_loss, want, want_g, shares = G.value_and_grad(x, y, Rr, bool(clamp), scale)
    nan = float("nan")
    xb = torch.full((Cn, H, rs), nan)
    xb[..., :W] = x[0]
    prefill = torch.full((Cn, H, rs), nan)
    g = torch.Generator().manual_seed(2)
    prefill[..., :W] = torch.randn(Cn, H, W, generator=g) * float(want.abs().max())
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("6i", H, W, rs, Cn, clamp, vec) + struct.pack("f", Rr) + struct.pack("d", scale))
        f.write(xb.numpy().tobytes() + y[0].contiguous().numpy().tobytes() + prefill.numpy().tobytes())
    subprocess.run([emulator, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, capture_output=True)
    b = open(tmp_path / "out.bin", "rb").read()
    loss, gm = struct.unpack("f", b[:4])[0], struct.unpack("d", b[4:12])[0]
    gx = torch.from_numpy(np.frombuffer(b[12:12 + 4 * Cn * H * rs], dtype=np.float32).copy()).view(Cn, H, rs)
    assert torch.equal(gx[..., W:].view(torch.int32), prefill[..., W:].view(torch.int32))          # outside [H, W]: bit-unchanged
    if float(want_g) == 0.0:
        assert gm == 0.0 and loss == 0.0 and torch.equal(gx.view(torch.int32), prefill.view(torch.int32))
        return
    assert float(want_g) >= 1e-3
    got = gx[None, :, :, :W].double()
    nbad, ratio = gate(got, want, prefill[None, :, :, :W].double())
    print(f"emulated kernels {H}x{W} vec {vec}: largest |got - ref| / bound {ratio:.4f}; value {loss:.9e} against {float(want_loss):.9e}; "
          f"GMSD {gm:.15f}; shares {shares}")
    assert nbad == 0 and ratio <= 1.0, (nbad, ratio)
    assert abs(gm - float(want_g)) <= 1e-12 * float(want_g)
    assert abs(loss - float(want_loss)) <= 1.2e-7 * abs(float(want_loss))
    keep = G.sector(shape)[0]
    if clamp:
        keep = keep | (x[0] < 0) | (x[0] > Rr)
    assert torch.equal(gx[..., :W][keep].view(torch.int32), prefill[..., :W][keep].view(torch.int32))
