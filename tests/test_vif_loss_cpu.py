"""CPU tests (no GPU) of the VIF loss term (TrainStep(lambda_vif=...), m2t_vif_loss / m2t_vif_loss_tensor): the fp64 restatement the GPU
tests compare the kernels with (tests/vif_loss_ref.py) -- its analytic gradient against torch autograd, its pyramid against
F.conv2d(...)[..., ::2, ::2], the size chain and the special values -- the C ABI table of include/m2t_vif.h, TrainStep's argument
validation and call sequence, the checkpoint entry, and the kernel text run on host threads (tests/vif_emulate.cpp) under the gate of
the GPU test."""
import contextlib
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from m2trans_amd import _lib as L
from tests import vif_loss_ref as V

N0 = L.VIF_SIGMA_N_SQ          # the library's default sigma_n_sq (2.0): the restatement is exercised at the value the step uses
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape,R,clamp,n", [((1, 1, 41, 41), 1.0, False, N0), ((2, 3, 42, 57), 255.0, True, N0),
                                             ((1, 3, 48, 61), 1.0, True, 0.7)], ids=["41", "rgb-255-clamp", "48x61-sigma"])
def test_analytic_gradient_equals_autograd_of_the_restatement_in_fp64(shape, R, clamp, n):
    """The coefficient maps, the transposed filters and the adjoint of (filter, decimate) against autograd of `vif` on the mixed family
    (dead, clamped and open entries all present): the difference is rounding, <= 1e-10 of the largest entry."""
    x, y = V.mixed_pair(shape, seed=3, R=R)
    leaf = x.double().clone().requires_grad_(True)
    v = V.vif(V.luminance(leaf, R, clamp), V.luminance(y, R, False), n)
    (0.7 * (1.0 - v).sum()).backward()
    loss, grad, vv, shares = V.value_and_grad(x, y, R, clamp, 0.7, n)
    assert min(shares[0].values()) > 0, shares[0]
    assert float((vv - v.detach()).abs().max()) <= 1e-14 and abs(float(loss) - 0.7 * float((1.0 - v.detach()).sum())) <= 1e-14
    assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    err = float((grad - leaf.grad).abs().max() / leaf.grad.abs().max())
    print(f"{shape}: analytic against autograd, {err:.3e} of the largest entry; shares at scale 0 {shares[0]}")
    assert err <= 1e-10, err
    if clamp:
        out = (x < 0) | (x > R)
        assert int(out.sum()) > 0 and int(torch.count_nonzero(grad[out])) == 0


def test_pyramid_is_the_valid_filter_then_every_second_sample():
    g = torch.Generator().manual_seed(5)
    t = torch.rand(2, 48, 61, generator=g, dtype=torch.float64)
    levels = V.pyramid(t)
    cur = t
    for s in range(1, V.SCALES):
        k = V.taps(s)
        assert k.numel() == (17, 9, 5, 3)[s] and abs(float(k.sum()) - 1.0) <= 1e-15 and torch.equal(k, k.flip(0))
        cur = F.conv2d(cur[:, None], torch.outer(k, k)[None, None])[:, 0, ::2, ::2]
        assert cur.shape == levels[s].shape and float((cur - levels[s]).abs().max()) <= 1e-14
        # the adjoint: <down(t), r> == <t, down_t(r)>
        fine = levels[s - 1]
        r = torch.rand(levels[s].shape, generator=g, dtype=torch.float64)
        assert abs(float((V.down(fine, s) * r).sum() - (fine * V.down_t(r, s, *fine.shape[-2:])).sum())) <= 1e-11
    n = 17
    ref = torch.exp(-(torch.arange(n, dtype=torch.float64) - 8.0) ** 2 / (2.0 * (n / 5.0) ** 2))
    assert float((V.taps(0) - ref / ref.sum()).abs().max()) <= 1e-17


def test_size_chain_from_41_gives_maps_25_9_3_1():
    from m2trans_amd import _lib
    from m2trans_amd.train_step import vif_size_supported
    levels = V.pyramid(torch.zeros(1, 41, 41, dtype=torch.float64))
    assert [t.shape[-1] for t in levels] == [41, 17, 7, 3]
    assert [t.shape[-1] - V.win_len(s) + 1 for s, t in enumerate(levels)] == [25, 9, 3, 1]
    assert V.MIN_SIDE == 41 == _lib.VIF_MIN_SIDE and _lib.VIF_SIGMA_N_SQ == 2.0
    assert vif_size_supported(41, 41) and not vif_size_supported(40, 400) and not vif_size_supported(400, 40)
    src = open(os.path.join(ROOT, "m2trans_amd", "csrc", "m2t_vif_tile.h")).read()
    assert "MIN_SIDE = 41" in src and "EPS = 1e-8" in src


def test_special_values():
    y = V.smooth((1, 3, 48, 61), 1).float()
    assert N0 == 2.0 and abs(float(V.value_and_grad(y, y, sigma_n_sq=N0)[2]) - 1.0) <= 1e-8                       # x = y (the value only: sv_raw sits at EPS)
    assert 1.05 < float(V.value_and_grad(1.5 * y, y)[2]) < 1.3                       # a contrast-enhanced x exceeds 1
    assert float(V.value_and_grad(1.5 * y, y, scale=2.0)[0]) < 0                     # ... and the term is negative, unclipped
    assert float(V.value_and_grad(torch.full_like(y, 0.3), y)[2]) < 1e-9             # a constant x
    flat = torch.full_like(y, 0.4)
    loss, grad, v, shares = V.value_and_grad(0.5 * flat, flat)
    assert float(v) == 1.0 and float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0     # both flat: exactly 1, exact zeros
    assert all(sh["dead"] == 1.0 for sh in shares)


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_decide_sizes_and_bad_arguments_on_the_host():
    from m2trans_amd import _lib
    lib = _lib.load()
    bad_off = C.c_size_t(-1).value
    assert lib.m2t_vif_loss_scratch_bytes(2, 3, 40, 400) == 0 and lib.m2t_vif_loss_scratch_bytes(2, 3, 400, 40) == 0
    assert lib.m2t_vif_loss_scratch_bytes(0, 3, 64, 64) == 0 and lib.m2t_vif_loss_scratch_bytes(65536, 3, 64, 64) == 0
    assert lib.m2t_vif_loss_scratch_bytes(1, 2, 64, 64) == 0 and lib.m2t_vif_loss_scratch_bytes(1, 4, 64, 64) == 0
    # 41 x 41, one image: record 4; tiles (9 + 4 + 1 + 1) x 2; three sets of levels 17^2 + 7^2 + 3^2 (the channel count changes nothing)
    levels = 17 * 17 + 7 * 7 + 3 * 3
    for ch in (1, 3):
        assert lib.m2t_vif_loss_scratch_bytes(1, ch, 41, 41) == 8 * (4 + 30 + 3 * levels)
    assert lib.m2t_vif_loss_scratch_bytes(2, 3, 41, 41) == 2 * 8 * (4 + 30 + 3 * levels)
    assert lib.m2t_vif_loss_scratch_offset(1, 1, 41, 41, 0, 0) == 0
    assert lib.m2t_vif_loss_scratch_offset(1, 1, 41, 41, 1, 0) == 8 * 4
    assert lib.m2t_vif_loss_scratch_offset(1, 1, 41, 41, 1, 1) == 8 * (4 + 18)
    assert lib.m2t_vif_loss_scratch_offset(1, 1, 41, 41, 2, 1) == 8 * (4 + 30)
    assert lib.m2t_vif_loss_scratch_offset(1, 1, 41, 41, 3, 1) == 8 * (4 + 30 + levels)
    assert lib.m2t_vif_loss_scratch_offset(1, 1, 41, 41, 4, 3) == 8 * (4 + 30 + 3 * levels - 9)
    for bad in ((1, 1, 40, 41, 0, 0), (1, 2, 41, 41, 0, 0), (1, 1, 41, 41, 2, 0), (1, 1, 41, 41, 5, 1), (1, 1, 41, 41, 1, 4), (1, 1, 41, 41, 1, -1)):
        assert lib.m2t_vif_loss_scratch_offset(*bad) == bad_off, bad
    one = C.c_void_p(8)                                              # a non-null pointer that is never followed
    call = lambda **kw: lib.m2t_vif_loss_tensor(*[kw.get(k, v) for k, v in (
        ("x", one), ("y", one), ("B", 1), ("C", 3), ("H", 48), ("W", 64), ("xs", 3 * 48 * 64), ("rs", 64), ("dr", 1.0), ("n", 2.0), ("clamp", 1),
        ("scale", 1.0), ("gx", None), ("loss", one), ("per", None), ("acc", 0), ("scratch", one), ("stream", None))])
    for bad in (dict(x=None), dict(y=None), dict(loss=None), dict(scratch=None), dict(H=40), dict(W=40), dict(H=10), dict(dr=0.0),
                dict(dr=-1.0), dict(dr=float("nan")), dict(dr=float("inf")), dict(n=0.0), dict(n=-2.0), dict(n=float("nan")),
                dict(n=float("inf")), dict(rs=63), dict(xs=3 * 48 * 64 - 3), dict(xs=3 * 48 * 64 + 1), dict(B=0), dict(B=65536),
                dict(C=2, xs=2 * 48 * 64), dict(C=4, xs=4 * 48 * 64)):
        assert call(**bad) == -2, bad
    assert call(H=40) == -2 and b"at least 41" in lib.m2t_last_error_string()
    assert call(C=2, xs=2 * 48 * 64) == -2 and b"1 or 3" in lib.m2t_last_error_string()
    assert lib.m2t_vif_loss(None, None, 1.0, 1.0, 1.0, 2.0, None, 0, None, None, None) == -2


def test_python_entries_refuse_host_tensors_small_images_and_bad_arguments():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import VIFLoss, vif_loss
    from m2trans_amd.metrics import vif_device
    x = torch.zeros(1, 3, 48, 48)
    for fn in (vif_loss, vif_device, VIFLoss()):
        with pytest.raises(M2TError):
            fn(x, x)                                                 # host tensors: no fallback
        with pytest.raises(M2TError):
            fn(x, x[..., :40])
    # (the remaining checks come before the device check, so they can be seen here)
    fake = types.SimpleNamespace(dim=lambda: 4, shape=torch.Size((1, 3, 48, 48)), is_cuda=True, requires_grad=False)
    for kw in (dict(data_range=0.0), dict(data_range=float("nan")), dict(sigma_n_sq=0.0), dict(sigma_n_sq=-1.0), dict(sigma_n_sq=float("inf"))):
        with pytest.raises(M2TError, match="finite number > 0"):
            vif_loss(fake, fake, **kw)
    two = types.SimpleNamespace(dim=lambda: 4, shape=torch.Size((1, 2, 48, 48)), is_cuda=True, requires_grad=False)
    with pytest.raises(M2TError, match="1 or 3 channels"):
        vif_loss(two, two)
    small = types.SimpleNamespace(dim=lambda: 4, shape=torch.Size((1, 3, 40, 48)), is_cuda=True, requires_grad=False)
    with pytest.raises(M2TError, match="at least 41"):
        vif_device(small, small)


# ------------------------------------------------------------------------------------------------------------- TrainStep
def test_lambda_vif_resolver_and_default():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep, resolve_lambda_vif
    assert inspect.signature(TrainStep.__init__).parameters["lambda_vif"].default == 0.0
    assert resolve_lambda_vif(0) == 0.0 and resolve_lambda_vif(0.05) == 0.05 and resolve_lambda_vif("0.5") == 0.5
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), None, "much"):
        with pytest.raises(M2TError):
            resolve_lambda_vif(bad)
    with pytest.raises(M2TError):
        TrainStep(None, lambda_vif=-1.0)


def test_set_lambda_vif_refuses_a_change_inside_an_accumulation_cycle():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    ts = TrainStep.__new__(TrainStep)
    ts.accum_steps, ts.micro_count, ts.vif_loss, ts._vif_scratch = 2, 1, None, {}
    with pytest.raises(M2TError, match="accumulation cycle"):
        ts.set_lambda_vif(0.0)
    ts.micro_count = 0
    ts.set_lambda_vif(0.0)
    assert ts.lambda_vif == 0.0 and ts.vif_loss is None and ts._vif_scratch == {}


def test_size_is_refused_before_any_launch():
    """_scratch_for refuses a small SR image on the host: no library call is made (lib = None would raise otherwise)."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import _TERM, TrainStep
    ts = TrainStep.__new__(TrainStep)
    ts._vif_scratch = {}
    with pytest.raises(M2TError, match="at least 41"):
        ts._scratch_for(_TERM["vif"], None, torch.zeros(2, 3, 40, 64))


class _Calls:
    """A stand-in for the loaded library: records the entry points in call order, every call succeeds."""

    def __init__(self):
        self.names, self.args = [], {}

    def __getattr__(self, name):
        def fn(*a):
            self.names.append(name)
            self.args[name] = a
            return 1 << 20 if name.endswith("scratch_bytes") else 0
        return fn


def _host_step(monkeypatch, **terms):
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
    ts.model, ts.micro_count, ts.accum_steps, ts.world_size = model, 0, 1, 1
    ts.semantic_loss, ts.lambda_clip, ts.lambda_l1 = None, 0.0, 1.0
    ts.grads, ts.micro_grads, ts.l1_loss, ts.micro_loss = torch.zeros(4), None, torch.zeros(1), None
    ts.set_pixel_loss("l1", None)
    ts.ssim_loss = ts.msssim_loss = ts.fft_loss = None
    ts._ssim_scratch, ts._msssim_scratch, ts._fft_scratch, ts.fft_norm = {}, {}, {}, "backward"
    ts.lambda_ssim, ts.lambda_msssim, ts.lambda_fft = 0.0, 0.0, 0.0
    for k, v in terms.items():
        if k != "lambda_vif":
            setattr(ts, k, v)
            setattr(ts, k.replace("lambda_", "") + "_loss", torch.zeros(1))
    if "lambda_vif" in terms:
        ts.vif_loss, ts._vif_scratch = None, {}
        ts.set_lambda_vif(terms["lambda_vif"])
    ts.forward_backward(torch.zeros(2, 3, 96, 96), torch.zeros(2, 3, 192, 192))
    return ts, calls


def test_lambda_vif_zero_issues_todays_call_sequence(monkeypatch):
    today = ["m2t_forward", "m2t_l1_loss_deferred", "m2t_backward"]
    _, bare = _host_step(monkeypatch)                                    # a step object that knows nothing of the term
    ts, zero = _host_step(monkeypatch, lambda_vif=0.0)
    assert bare.names == today and zero.names == today
    assert ts.vif_loss is None and ts._vif_scratch == {}                 # nothing allocated


def test_lambda_vif_takes_the_materialised_seed_last_before_the_backward(monkeypatch):
    from m2trans_amd import _lib
    ts, on = _host_step(monkeypatch, lambda_vif=0.05)
    assert on.names == ["m2t_vif_loss_scratch_bytes", "m2t_forward", "m2t_l1_loss", "m2t_vif_loss", "m2t_backward"]
    a = on.args["m2t_vif_loss"]
    assert a[2] == 0.05 and a[3] == 2.0 and a[4] == 1.0 and a[5] == _lib.VIF_SIGMA_N_SQ and a[7] == 0     # weight, divisor = B, R, n, store
    assert list(ts._vif_scratch) == [(2, 192, 192)]
    _, every = _host_step(monkeypatch, lambda_ssim=0.1, lambda_msssim=0.16, lambda_fft=0.1, lambda_vif=0.05)
    order = [n for n in every.names if not n.endswith("scratch_bytes")]
    assert order == ["m2t_forward", "m2t_l1_loss", "m2t_ssim_loss", "m2t_msssim_loss", "m2t_fft_loss", "m2t_vif_loss", "m2t_backward"]


# ------------------------------------------------------------------------------------------------------------- checkpoint
def _model():
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))


class _Step:
    """The flat-buffer part of TrainStep on the CPU, with the pixel loss and the weights of the optional terms."""

    def __init__(self, m, pixel_loss="l1", pixel_loss_param=None, lambda_vif=0.0, lambda_ssim=0.0, lambda_msssim=0.0, lambda_fft=0.0,
                 step_count=7, lr=5e-5):
        from m2trans_amd.train_step import TrainStep
        g = torch.Generator().manual_seed(step_count)
        self.exp_avg = torch.randn(m.flat_params.shape, generator=g)
        self.exp_avg_sq = torch.rand(m.flat_params.shape, generator=g)
        self.step_count, self.lr, self.scheduler_last_epoch = step_count, lr, 0
        self.micro_count, self.accum_steps = 0, 1
        self.lambda_ssim, self.lambda_msssim, self.lambda_fft, self.fft_norm = lambda_ssim, lambda_msssim, lambda_fft, "backward"
        TrainStep.set_pixel_loss(self, pixel_loss, pixel_loss_param)
        self.set_lambda_vif(lambda_vif)

    def set_pixel_loss(self, name, param=None):
        from m2trans_amd.train_step import TrainStep
        TrainStep.set_pixel_loss(self, name, param)

    def set_lambda_ssim(self, value):
        self.lambda_ssim = float(value)

    def set_lambda_msssim(self, value):
        self.lambda_msssim = float(value)

    def set_lambda_fft(self, value, norm=None):
        self.lambda_fft = float(value)

    def set_lambda_vif(self, value):
        from m2trans_amd.train_step import resolve_lambda_vif
        self.lambda_vif = resolve_lambda_vif(value)

    def set_lr(self, lr):
        self.lr = lr


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    return type(a) is type(b) and a == b


def test_checkpoint_without_the_term_is_todays_dict():
    from m2trans_amd.checkpoint import export_checkpoint
    m = _model()
    keys = ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict"]
    bare = types.SimpleNamespace(lr=5e-5, step_count=7, exp_avg=_Step(m).exp_avg, exp_avg_sq=_Step(m).exp_avg_sq)     # knows no lambda_vif
    zero = export_checkpoint(m, _Step(m, lambda_vif=0.0), epoch=3)
    assert list(zero) == keys and _same(zero, export_checkpoint(m, bare, epoch=3))
    # the other terms with lambda_vif = 0: the entries of before, without the key
    assert export_checkpoint(m, _Step(m, "charbonnier", 1e-3), epoch=3)["m2t_loss"] == {"pixel_loss": "charbonnier", "param": 1e-3}
    assert export_checkpoint(m, _Step(m, lambda_msssim=0.16), epoch=3)["m2t_loss"] == {"pixel_loss": "l1", "param": None, "lambda_msssim": 0.16}


@pytest.mark.parametrize("name,param,entry", [("l1", None, {"pixel_loss": "l1", "param": None, "lambda_vif": 0.05}),
                                              ("sl1", 0.25, {"pixel_loss": "smooth_l1", "param": 0.25, "lambda_vif": 0.05})])
def test_checkpoint_entry_carries_lambda_vif_and_round_trips(name, param, entry):
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model()
    src = _Step(m, name, param, lambda_vif=0.05)
    ck = export_checkpoint(m, src, epoch=3)
    assert list(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict", "m2t_loss"]
    assert ck["m2t_loss"] == entry and list(ck["m2t_loss"]) == list(entry)
    for start in (0.0, 0.7):                                                      # whatever the importing step was built with
        dst = _Step(_model(), "mse", None, lambda_vif=start, step_count=1)
        assert import_checkpoint(ck, _model(), dst) == 4
        assert dst.lambda_vif == 0.05 and (dst.pixel_loss, dst.pixel_loss_param) == (src.pixel_loss, src.pixel_loss_param)
        assert dst.step_count == 7 and torch.equal(dst.exp_avg, src.exp_avg)
    # a file whose entry has no lambda_vif (saved with 0), and one without an entry, leave the importing step's weight alone
    dst = _Step(_model(), lambda_vif=0.7)
    import_checkpoint(export_checkpoint(m, _Step(m, "mse"), epoch=3), _model(), dst)
    assert dst.lambda_vif == 0.7 and dst.pixel_loss == "mse"
    import_checkpoint(export_checkpoint(m, _Step(m), epoch=3), _model(), dst)
    assert dst.lambda_vif == 0.7
    # with every other term next to it: the key comes after the existing ones
    every = export_checkpoint(m, _Step(m, lambda_vif=0.05, lambda_ssim=0.1, lambda_msssim=0.16, lambda_fft=0.2), epoch=3)["m2t_loss"]
    assert list(every) == ["pixel_loss", "param", "lambda_ssim", "lambda_msssim", "lambda_fft", "fft_norm", "lambda_vif"]
    # a plain object without the setters receives the attribute
    plain = types.SimpleNamespace(lr=1.0, step_count=0, exp_avg=torch.zeros_like(m.flat_params), exp_avg_sq=torch.zeros_like(m.flat_params),
                                  scheduler_last_epoch=0, set_lr=lambda lr: None)
    import_checkpoint(ck, _model(), plain)
    assert plain.lambda_vif == 0.05


# ------------------------------------------------------------------------------------------------------------- host emulation
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    import shutil
    import subprocess
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"), shutil.which("clang++"), shutil.which("g++"))
                if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("vif") / "vif_emulate")
    subprocess.run([cxx, "-x", "c++", "-std=c++20", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "emulate_hip"),
                    "-I", os.path.join(ROOT, "m2trans_amd", "csrc"), os.path.join(ROOT, "tests", "vif_emulate.cpp"), "-o", exe, "-lpthread"],
                   check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("H,W,rs,Cn,Rr,clamp", [(41, 41, 41, 1, 1.0, 0), (44, 157, 160, 3, 255.0, 1)], ids=["41x41", "44x157-two-tiles-per-scale"])
def test_kernel_text_emulated_on_the_host_meets_the_gpu_gate(emulator, tmp_path, H, W, rs, Cn, Rr, clamp):
    """csrc/m2t_vif_tile.h -- the text the kernels run -- on host threads (tests/vif_emulate.cpp), the kernel's own sum order: the
    smallest size, and one with two tiles on every scale (level widths 157 / 75 / 36 / 17), RGB, R = 255, clamp on, x in a NaN-filled
    buffer with a longer row.  The pyramid within 1e-12, the gradient within the gate of the GPU test
    (1e-6 |ref| + 1e-7 max |ref| + 6e-8 |prefill + ref|), the value within fp32 rounding, nothing written outside [H, W]."""
    import struct
    import subprocess
    import numpy as np
    scale, nn = 0.37, N0
    x, y = V.mixed_pair((1, Cn, H, W), seed=10, R=Rr)
    want_loss, want, want_v, shares = V.value_and_grad(x, y, Rr, bool(clamp), scale, nn)
    assert min(shares[0].values()) > 0, shares[0]
    if W > 150:
        assert V.pyramid(torch.zeros(1, H, W, dtype=torch.float64))[3].shape[-1] > 16
    g = torch.Generator().manual_seed(7)
    prefill = (torch.randn(Cn, H, rs, generator=g) * float(want.abs().max())).float()
    xb = torch.full((Cn, H, rs), float("nan"))
    xb[..., :W] = x[0]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("5i", H, W, rs, Cn, clamp) + struct.pack("f", Rr) + struct.pack("2d", scale, nn))
        f.write(xb.numpy().tobytes() + y[0].numpy().tobytes() + prefill.numpy().tobytes())
    subprocess.run([emulator, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, capture_output=True)
    b = open(tmp_path / "out.bin", "rb").read()
    loss, vif = struct.unpack("f", b[:4])[0], struct.unpack("d", b[4:12])[0]
    gx = torch.from_numpy(np.frombuffer(b[12:12 + 4 * Cn * H * rs], dtype=np.float32).copy()).view(Cn, H, rs)
    off = 12 + 4 * Cn * H * rs
    for level in V.pyramid(V.luminance(x, Rr, bool(clamp)))[1:]:
        got = torch.from_numpy(np.frombuffer(b[off:off + 8 * level.numel()], dtype=np.float64).copy()).view(level.shape)
        off += 8 * level.numel()
        assert float((got - level).abs().max()) <= 1e-12 * float(level.abs().max()), tuple(level.shape)
    assert off == len(b)
    total = prefill[..., :W].double() + want[0]
    bound = 1e-6 * want[0].abs() + 1e-7 * want.abs().max() + 6e-8 * total.abs()
    ratio = float(((gx[..., :W].double() - total).abs() / bound).max())
    excess = ((gx[..., :W].double() - total).abs() - 6e-8 * total.abs()).clamp(min=0.0)      # what the fp32 rounding does not explain
    tight = float((excess / (1e-6 * want[0].abs() + 1e-7 * want.abs().max())).max())
    print(f"emulated kernels {H}x{W}: largest |got - ref| / bound {ratio:.4f}; beyond the fp32 rounding term, against the first two terms "
          f"{tight:.3e}; value {loss:.9e} against {float(want_loss):.9e}; VIF {vif:.15f}")
    assert ratio <= 1.0, ratio
    assert torch.equal(gx[..., W:].view(torch.int32), prefill[..., W:].view(torch.int32))
    assert abs(loss - float(want_loss)) <= 1e-6 * abs(float(want_loss)) and abs(vif - float(want_v)) <= 1e-12 * float(want_v)
