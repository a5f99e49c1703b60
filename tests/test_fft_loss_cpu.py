"""CPU tests (no GPU) of the frequency-domain loss term (TrainStep(lambda_fft=...), include/m2t_spectral.h): the fp64 restatement the
GPU tests compare the kernels with (tests/fft_loss_ref.py) against torch.fft and torch autograd, the second header against its
signature table and the library's symbols, the size rule and the argument checks of the entry points (decided on the host, before
any launch), TrainStep's argument validation and the checkpoint entry."""
import ctypes as C
import inspect
import math
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from tests import fft_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W), seed of the input recipe: the pairs the GPU tests use, with the smallest spectral component over the RMS measured on the CPU
CASES = [((16, 16), 0), ((24, 32), 1), ((32, 48), 0), ((36, 64), 4), ((48, 24), 0), ((96, 64), 0)]


# ------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("shape,seed", CASES)
def test_reference_value_is_l1_of_torch_rfft2_in_fp64(shape, seed):
    x, y = R.inputs(*shape, seed)
    xd, yd = x.double(), y.double()
    want = F.l1_loss(torch.view_as_real(torch.fft.rfft2(xd)), torch.view_as_real(torch.fft.rfft2(yd)))
    got, _ = R.value_and_grad(x, y)
    assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want)), (float(got), float(want))


@pytest.mark.parametrize("shape,seed", CASES)
def test_reference_gradient_is_autograd_once_the_self_conjugate_signs_are_zeroed(shape, seed):
    """The formula (half-spectrum inverse-direction DFT of the signs, no Hermitian doubling) against autograd of torch.fft in fp64,
    with the four self-conjugate imaginary parts masked in the autograd graph too: 1e-12 of the largest entry."""
    H, W = shape
    x, y = R.inputs(H, W, seed)
    leaf = x.double().clone().requires_grad_(True)
    keep = torch.ones(H, W // 2 + 1, 2, dtype=torch.float64)
    keep[..., 1][R.self_conjugate_mask(H, W)] = 0.0
    (torch.view_as_real(torch.fft.rfft2(leaf - y.double())) * keep).abs().mean().backward()
    _, got = R.value_and_grad(x, y)
    assert float(leaf.grad.abs().max()) > 0
    err = float((got - leaf.grad).abs().max() / leaf.grad.abs().max())
    assert err <= 1e-12, err


def test_reference_ortho_is_backward_over_sqrt_hw_and_the_clamp_masks_the_gradient():
    H, W = 24, 32
    x, y = R.inputs(H, W, 1, push_seed=100)
    s = 1.0 / math.sqrt(H * W)
    for clamp in (False, True):
        vb, gb = R.value_and_grad(x, y, 1.0, clamp, None, "backward")
        vo, go = R.value_and_grad(x, y, 1.0, clamp, None, "ortho")
        assert abs(float(vo) - s * float(vb)) <= 1e-14 * abs(float(vb))
        assert float((go - s * gb).abs().max()) <= 1e-14 * float(gb.abs().max())
    outside = (x < 0) | (x > 1)
    assert 0.05 < float(outside.double().mean()) < 0.15
    assert int(torch.count_nonzero(gb[outside])) == 0 and int(torch.count_nonzero(gb[~outside])) > 0
    # data_range R and a weight / divisor, against autograd of the definition through the clamp and the padded layout
    Rr, w = 2.0, 0.3
    pre = torch.zeros(2, 3, 32, 40, dtype=torch.float64)
    pre[..., :H, :W] = x.double() * Rr
    hr = y.double() * Rr
    leaf = pre.clone().requires_grad_(True)
    keep = torch.ones(H, W // 2 + 1, 2, dtype=torch.float64)
    keep[..., 1][R.self_conjugate_mask(H, W)] = 0.0
    D = torch.view_as_real(torch.fft.rfft2(leaf[..., :H, :W].clamp(0.0, Rr) / Rr - hr / Rr)) * keep
    want = w * D.abs().sum() / (5.0 * D.numel())
    want.backward()
    loss, seed = R.loss_and_seed(pre, hr, weight=w, divisor=5.0 * D.numel(), R=Rr)
    assert abs(float(loss) - float(want.detach())) <= 1e-14
    assert float((seed - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max())
    assert int(torch.count_nonzero(seed[..., H:, :])) == 0 and int(torch.count_nonzero(seed[..., :, W:])) == 0


@pytest.mark.parametrize("shape,seed", CASES)
def test_the_listed_inputs_stay_off_the_kink(shape, seed):
    """Every non-self-conjugate component of the fp64 spectrum is at least 1e-5 of their RMS (the GPU tests assert it again on what
    they run); the self-conjugate imaginary parts of the reference are exactly 0."""
    x, y = R.inputs(*shape, seed)
    assert R.kink_margin(x.double() - y.double()) >= 1e-5
    D = R.spectrum(x.double() - y.double())
    assert int(torch.count_nonzero(D.imag[..., R.self_conjugate_mask(*shape)])) == 0


# ------------------------------------------------------------------------------------------------------------- C ABI
def _supported(n):
    if n < 8 or n > 2048 or n % 2:
        return False
    while n % 2 == 0:
        n //= 2
    while n % 3 == 0:
        n //= 3
    return n == 1


def test_size_rule_is_decided_on_the_host():
    from m2trans_amd import _lib
    from m2trans_amd.train_step import fft_size_supported
    lib = _lib.load()
    for H, W in ((10, 16), (40, 56), (4096, 16), (16, 10), (16, 4096), (6, 16), (16, 27), (160, 224)):
        assert lib.m2t_fft_loss_scratch_bytes(2, 3, H, W) == 0, (H, W)
    assert lib.m2t_fft_loss_scratch_bytes(0, 3, 16, 16) == 0 and lib.m2t_fft_loss_scratch_bytes(2, 0, 16, 16) == 0
    # the half spectrum (fp32 complex) + one double per strip of the column pass and plane
    assert lib.m2t_fft_loss_scratch_bytes(1, 1, 16, 16) == 8 * 16 * 9 + 8 * 1
    assert lib.m2t_fft_loss_scratch_bytes(2, 3, 96, 64) == 6 * (8 * 96 * 33 + 8 * 3)
    assert lib.m2t_fft_loss_scratch_bytes(1, 3, 2048, 2048) == 3 * (8 * 2048 * 1025 + 8 * 513)
    for n in range(0, 2100):
        assert fft_size_supported(n) == _supported(n), n
        assert (lib.m2t_fft_loss_scratch_bytes(1, 1, n, 16) > 0) == _supported(n), n
        assert (lib.m2t_fft_loss_scratch_bytes(1, 1, 16, n) > 0) == _supported(n), n
    assert all(_supported(n) for n in (192, 256, 384, 512, 576, 768))          # the training patches of the shipped configs


def test_entry_points_refuse_bad_arguments_without_a_device():
    from m2trans_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(8)                                                          # a non-null pointer that is never followed
    call = lambda **kw: lib.m2t_fft_loss_tensor(*[kw.get(k, v) for k, v in (
        ("x", one), ("y", one), ("B", 1), ("C", 3), ("H", 16), ("W", 16), ("xs", 3 * 256), ("rs", 16), ("dr", 1.0), ("clamp", 1), ("norm", 0),
        ("scale", 1.0), ("gx", None), ("loss", one), ("acc", 0), ("scratch", one), ("stream", None))])
    for bad in (dict(x=None), dict(y=None), dict(loss=None), dict(scratch=None), dict(H=10), dict(W=10), dict(H=15), dict(W=17), dict(H=40),
                dict(W=56), dict(H=4096), dict(H=6), dict(dr=0.0), dict(dr=-1.0), dict(dr=float("nan")), dict(dr=float("inf")), dict(norm=2),
                dict(norm=-1), dict(rs=15), dict(xs=3 * 255), dict(xs=3 * 256 + 1), dict(B=0), dict(C=0), dict(B=65536),
                dict(scale=float("nan"))):
        assert call(**bad) == -2, bad
    assert b"2^a * 3^b" in (call(H=40), lib.m2t_last_error_string())[1]
    rf = lambda **kw: lib.m2t_rfft2(*[kw.get(k, v) for k, v in (("x", one), ("out", one), ("planes", 1), ("H", 16), ("W", 16), ("norm", 0),
                                                                  ("stream", None))])
    for bad in (dict(x=None), dict(out=None), dict(planes=0), dict(planes=65536), dict(H=10), dict(W=40), dict(H=9), dict(norm=2)):
        assert rf(**bad) == -2, bad
    assert lib.m2t_fft_loss(None, None, 1.0, 1.0, 1.0, 0, None, 0, None, None, None) == -2


# ------------------------------------------------------------------------------------------------------------- TrainStep
def test_lambda_fft_resolvers_and_defaults():
    from m2trans_amd._lib import FFT_NORMS, M2TError
    from m2trans_amd.train_step import TrainStep, resolve_fft_norm, resolve_lambda_fft
    params = inspect.signature(TrainStep.__init__).parameters
    assert params["lambda_fft"].default == 0.0 and params["fft_norm"].default == "backward"
    assert resolve_lambda_fft(0) == 0.0 and resolve_lambda_fft(0.1) == 0.1 and resolve_lambda_fft("0.5") == 0.5
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), None, "much"):
        with pytest.raises(M2TError):
            resolve_lambda_fft(bad)
    assert FFT_NORMS == {"backward": 0, "ortho": 1} == R.NORMS
    assert resolve_fft_norm("backward") == "backward" and resolve_fft_norm("Ortho") == "ortho"
    for bad in ("forward", "", None, 1):
        with pytest.raises(M2TError):
            resolve_fft_norm(bad)
    # the checks come before the model (None here) is looked at
    with pytest.raises(M2TError):
        TrainStep(None, lambda_fft=-1.0)
    with pytest.raises(M2TError):
        TrainStep(None, lambda_fft=0.0, fft_norm="forward")


def test_set_lambda_fft_refuses_a_change_inside_an_accumulation_cycle():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    ts = TrainStep.__new__(TrainStep)
    ts.accum_steps, ts.micro_count, ts.fft_loss, ts._fft_scratch, ts.fft_norm = 2, 1, None, {}, "backward"
    with pytest.raises(M2TError):
        ts.set_lambda_fft(0.0)
    ts.micro_count = 0
    ts.set_lambda_fft(0.0, "ortho")
    assert ts.lambda_fft == 0.0 and ts.fft_loss is None and ts.fft_norm == "ortho"
    ts.set_lambda_fft(0.0)
    assert ts.fft_norm == "ortho"                                                 # norm=None leaves it


def test_fft_loss_function_refuses_before_any_launch():
    """Host tensors, a y that requires grad, an unsupported size, an unknown norm: M2TError, no device needed to say so."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import FFTLoss, fft_loss
    x, y = torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16)
    with pytest.raises(M2TError, match="HIP device"):
        fft_loss(x, y)
    with pytest.raises(M2TError):
        fft_loss(x, y[:, :2])
    with pytest.raises(M2TError):
        FFTLoss(norm="forward")
    assert FFTLoss(2.0, "ortho").norm == "ortho"


# ------------------------------------------------------------------------------------------------------------- checkpoint
def _model():
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))


class _Step:
    """The flat-buffer part of TrainStep on the CPU, with the pixel loss and the weights of the two extra terms."""

    def __init__(self, m, pixel_loss="l1", pixel_loss_param=None, lambda_ssim=0.0, lambda_fft=0.0, fft_norm="backward", step_count=7, lr=5e-5):
        from m2trans_amd.train_step import TrainStep, resolve_lambda_ssim
        g = torch.Generator().manual_seed(step_count)
        self.exp_avg = torch.randn(m.flat_params.shape, generator=g)
        self.exp_avg_sq = torch.rand(m.flat_params.shape, generator=g)
        self.step_count, self.lr, self.scheduler_last_epoch = step_count, lr, 0
        self.micro_count, self.accum_steps = 0, 1
        TrainStep.set_pixel_loss(self, pixel_loss, pixel_loss_param)
        self.lambda_ssim = resolve_lambda_ssim(lambda_ssim)
        self.fft_norm = "backward"
        self.set_lambda_fft(lambda_fft, fft_norm)

    def set_pixel_loss(self, name, param=None):
        from m2trans_amd.train_step import TrainStep
        TrainStep.set_pixel_loss(self, name, param)

    def set_lambda_ssim(self, value):
        from m2trans_amd.train_step import resolve_lambda_ssim
        self.lambda_ssim = resolve_lambda_ssim(value)

    def set_lambda_fft(self, value, norm=None):
        from m2trans_amd.train_step import resolve_fft_norm, resolve_lambda_fft
        self.lambda_fft = resolve_lambda_fft(value)
        if norm is not None:
            self.fft_norm = resolve_fft_norm(norm)

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
    bare = types.SimpleNamespace(lr=5e-5, step_count=7, exp_avg=_Step(m).exp_avg, exp_avg_sq=_Step(m).exp_avg_sq)     # knows no lambda_fft
    zero = export_checkpoint(m, _Step(m, lambda_fft=0.0, fft_norm="ortho"), epoch=3)
    assert list(zero) == keys and _same(zero, export_checkpoint(m, bare, epoch=3))
    # the entries of before, without the new keys
    assert export_checkpoint(m, _Step(m, "charbonnier", 1e-3), epoch=3)["m2t_loss"] == {"pixel_loss": "charbonnier", "param": 1e-3}
    assert export_checkpoint(m, _Step(m, lambda_ssim=0.1), epoch=3)["m2t_loss"] == {"pixel_loss": "l1", "param": None, "lambda_ssim": 0.1}


@pytest.mark.parametrize("kw,entry", [
    (dict(lambda_fft=0.05), {"pixel_loss": "l1", "param": None, "lambda_fft": 0.05, "fft_norm": "backward"}),
    (dict(pixel_loss="sl1", pixel_loss_param=0.25, lambda_ssim=0.1, lambda_fft=0.05, fft_norm="ortho"),
     {"pixel_loss": "smooth_l1", "param": 0.25, "lambda_ssim": 0.1, "lambda_fft": 0.05, "fft_norm": "ortho"})])
def test_checkpoint_entry_carries_lambda_fft_and_round_trips(kw, entry):
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model()
    src = _Step(m, **kw)
    ck = export_checkpoint(m, src, epoch=3)
    assert list(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict", "m2t_loss"]
    assert ck["m2t_loss"] == entry and list(ck["m2t_loss"]) == list(entry)
    for start in (0.0, 0.7):                                                      # whatever the importing step was built with
        dst = _Step(_model(), "mse", None, lambda_fft=start, fft_norm="ortho" if entry["fft_norm"] == "backward" else "backward", step_count=1)
        assert import_checkpoint(ck, _model(), dst) == 4
        assert dst.lambda_fft == 0.05 and dst.fft_norm == entry["fft_norm"] and dst.lambda_ssim == src.lambda_ssim
        assert (dst.pixel_loss, dst.pixel_loss_param) == (src.pixel_loss, src.pixel_loss_param)
        assert dst.step_count == 7 and torch.equal(dst.exp_avg, src.exp_avg)
    # a file whose entry has no lambda_fft (saved with 0), and one without an entry, leave the importing step's term alone
    dst = _Step(_model(), lambda_fft=0.7, fft_norm="ortho")
    import_checkpoint(export_checkpoint(m, _Step(m, "mse"), epoch=3), _model(), dst)
    assert (dst.lambda_fft, dst.fft_norm, dst.pixel_loss) == (0.7, "ortho", "mse")
    import_checkpoint(export_checkpoint(m, _Step(m), epoch=3), _model(), dst)
    assert (dst.lambda_fft, dst.fft_norm) == (0.7, "ortho")
    # a plain object without the setters receives the attributes
    plain = types.SimpleNamespace(lr=1.0, step_count=0, exp_avg=torch.zeros_like(m.flat_params), exp_avg_sq=torch.zeros_like(m.flat_params),
                                  scheduler_last_epoch=0, set_lr=lambda lr: None)
    import_checkpoint(ck, _model(), plain)
    assert plain.lambda_fft == 0.05 and plain.fft_norm == entry["fft_norm"]


# ------------------------------------------------------------------------------------------------------------- the kernels' arithmetic, on the host
# csrc/m2t_fft.h holds the per-workgroup phases of the three kernels as functions of (workgroup, thread index, thread count);
# tests/fft_emulate.hip runs that text on the host (a loop over the thread index in place of the workgroup).  The gate is the GPU
# tests': 8 x the error of torch's own fp32 pipeline on the listed cases, capped at 2e-5.
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    import subprocess
    from m2trans_amd.build import _hipcc
    exe = str(tmp_path_factory.mktemp("fft_emulate") / "fft_emulate")
    cmd = [_hipcc(), "--offload-host-only", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "fft_emulate.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


_GATES = []


def _gates():
    if not _GATES:
        floors = [R.torch_fp32_floor(*R.inputs(*shape, seed)) for shape, seed in CASES]
        _GATES.extend(min(8.0 * max(f[i] for f in floors), 2e-5) for i in range(3))
    return _GATES


@pytest.mark.parametrize("case,clamp,norm,pad", [(0, 0, "backward", (0, 0)), (1, 1, "ortho", (8, 16)), (2, 0, "ortho", (0, 0)), (3, 1, "backward", (3, 5)),
                                                 (4, 0, "backward", (8, 16)), (5, 1, "ortho", (0, 0))])
def test_kernel_phases_on_the_host_against_fp64(emulator, tmp_path, case, clamp, norm, pad):
    import struct
    import subprocess
    import numpy as np
    (H, W), seed = CASES[case]
    x, y = R.inputs(H, W, seed, push_seed=100 + (case == 2) if clamp else None)
    B, Cn = x.shape[:2]
    margin = R.kink_margin((x.double().clamp(0, 1) if clamp else x.double()) - y.double())
    assert margin >= 1e-5, margin
    rows, rs = H + pad[0], W + pad[1]
    scale = 0.37 / (2 * B * Cn * H * (W // 2 + 1))
    xbuf = torch.full((B, Cn, rows, rs), float("nan"))
    xbuf[..., :H, :W] = x
    gbuf = torch.full((B, Cn, rows, rs), float("nan"))
    gbuf[..., :H, :W] = 0.0
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<8id", B, Cn, H, W, rows, rs, clamp, R.NORMS[norm], scale))
        for t in (xbuf, y, gbuf):
            f.write(t.contiguous().numpy().tobytes())
    assert subprocess.run([emulator, fin, fout]).returncode == 0
    raw = np.fromfile(fout, dtype=np.float32)
    n = B * Cn * rows * rs
    loss, got = float(raw[0]), torch.from_numpy(raw[1:1 + n].copy()).view(B, Cn, rows, rs)
    spec = torch.from_numpy(raw[1 + n:].copy()).view(B, Cn, H, W // 2 + 1, 2)
    want_loss, want = R.value_and_grad(x, y, 1.0, bool(clamp), scale, norm)
    g_spec, g_val, g_grad = _gates()
    err = float((got[..., :H, :W].double() - want).abs().max() / want.abs().max())
    verr = abs(loss - float(want_loss)) / abs(float(want_loss))
    want_spec = torch.view_as_real(torch.fft.rfft2(y.double(), norm=norm))
    serr = float((spec.double() - want_spec).abs().max() / want_spec.abs().max())
    print(f"{H}x{W} clamp {clamp} {norm}: gradient {err:.3e} (gate {g_grad:.3e}), value {verr:.3e} (gate {g_val:.3e}), spectrum {serr:.3e} (gate {g_spec:.3e})")
    assert err <= g_grad and verr <= g_val and serr <= g_spec, (err, verr, serr)
    inside = torch.zeros((B, Cn, rows, rs), dtype=torch.bool)
    inside[..., :H, :W] = True
    assert bool(torch.isnan(got[~inside]).all()), "an element outside [H, W] was written"
    if clamp:
        outside = (x < 0) | (x > 1)
        assert bool((got[..., :H, :W][outside].view(torch.int32) == 0).all())
    im = spec[..., 1][..., R.self_conjugate_mask(H, W)]
    assert bool((im.view(torch.int32) == 0).all()), "self-conjugate imaginary parts must be +0.0"
