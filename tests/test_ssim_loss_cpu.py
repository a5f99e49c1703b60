"""CPU tests (no GPU) of the SSIM loss term (TrainStep(lambda_ssim=...), m2t_ssim_loss / m2t_ssim_loss_tensor): the fp64
restatement the GPU tests compare the kernels with (tests/ssim_loss_ref.py) -- its analytic gradient against torch autograd, its
value against anchors and an independent scipy evaluation -- the C ABI table, TrainStep's argument validation, the checkpoint entry,
and the kernel text run on host threads (tests/ssim_emulate.cpp) under the gate of the GPU test."""
import ctypes as C
import inspect
import types

import pytest
import torch

from oracle import m2trans_oracle as O
from tests import ssim_loss_ref as R


def _pair(shape, seed=3):
    """fp64 images with structure and noise: x on both sides of [0, 1] is NOT needed here (the clamp is outside ssim_map)."""
    g = torch.Generator().manual_seed(seed)
    b, c, h, w = shape
    y = O.closed_form_image(b, c, h, w, phase=0.7, dtype=torch.float64)
    x = (O.closed_form_image(b, c, h, w, phase=0.2, dtype=torch.float64) + 0.05 * torch.randn(shape, generator=g, dtype=torch.float64))
    return x, y


def test_analytic_gradient_equals_autograd_of_the_restatement_in_fp64():
    """d sum(S) / dx as the kernel computes it (three coefficient maps through the transposed filter) against autograd of ssim_map:
    max difference <= 1e-12 of the largest entry (measured 6e-15)."""
    x, y = _pair((2, 3, 23, 31))
    leaf = x.clone().requires_grad_(True)
    R.ssim_map(leaf, y).sum().backward()
    got = R.dsum_dx(x, y)
    assert got.shape == x.shape and float(leaf.grad.abs().max()) > 0
    err = float((got - leaf.grad).abs().max() / leaf.grad.abs().max())
    assert err <= 1e-12, err


def test_loss_and_seed_equals_autograd_through_the_clamp_and_the_padded_layout():
    """loss_and_seed: weight / divisor, rgb_range R != 1, the clamp mask and the zero padding, against autograd of the definition."""
    g = torch.Generator().manual_seed(11)
    Rr, w = 2.0, 0.3
    pre = (torch.rand(2, 3, 24, 32, generator=g, dtype=torch.float64) * 1.6 - 0.3) * Rr
    hr = O.closed_form_image(2, 3, 21, 27, phase=0.4, dtype=torch.float64) * Rr
    leaf = pre.clone().requires_grad_(True)
    S = R.ssim_map(leaf[..., :21, :27].clamp(0.0, Rr) / Rr, hr / Rr)
    n = S.numel()
    want = w * (1.0 - S).sum() / (3.0 * n)
    want.backward()
    loss, seed = R.loss_and_seed(pre, hr, weight=w, divisor=3.0 * n, R=Rr)
    assert abs(float(loss) - float(want.detach())) <= 1e-14
    assert float((seed - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max())
    assert int(torch.count_nonzero(seed[..., 21:, :])) == 0 and int(torch.count_nonzero(seed[..., :, 27:])) == 0
    inner = pre[..., :21, :27]
    assert int(torch.count_nonzero(seed[..., :21, :27][(inner < 0) | (inner > Rr)])) == 0
    assert float(R.loss_and_seed(pre, hr, R=Rr)[0]) == pytest.approx(float(want.detach()) * 3.0 / w, rel=1e-13)       # default divisor: the mean


def test_identity_symmetry_and_constant_closed_form():
    x, y = _pair((2, 3, 40, 56))
    loss, grad = R.value_and_grad(y, y)
    assert abs(float(loss)) <= 1e-12 * y[..., 10:, 10:].numel()
    assert float(grad.abs().max()) <= 1e-9                      # rounding level (the map is flat at its maximum, 1)
    assert float((R.ssim_map(x, y) - R.ssim_map(y, x)).abs().max()) <= 1e-14
    # constant images: with the window's sum s (1 +- 1e-7 after the fp32 normalisation) every moment is closed-form
    a, b = 0.25, 0.75
    s = float(R.taps().sum()) ** 2
    m1, m2 = a * s, b * s
    s1, s2, s12 = a * a * s - m1 * m1, b * b * s - m2 * m2, a * b * s - m1 * m2
    want = ((2 * m1 * m2 + R.C1) / (m1 * m1 + m2 * m2 + R.C1)) * ((2 * s12 + R.C2) / (s1 + s2 + R.C2))
    got = R.ssim_map(torch.full((1, 3, 16, 20), a, dtype=torch.float64), torch.full((1, 3, 16, 20), b, dtype=torch.float64))
    assert got.shape == (1, 3, 6, 10) and float((got - want).abs().max()) <= 1e-12
    assert abs(want - (2 * a * b + R.C1) / (a * a + b * b + R.C1)) < 1e-4


def test_value_against_independent_scipy_float64():
    from scipy.ndimage import correlate1d
    x, y = _pair((2, 1, 64, 48))
    g = R.taps().numpy()

    def filt(t):      # 'valid' part of a separable correlation
        t = correlate1d(correlate1d(t, g, axis=0, mode="constant"), g, axis=1, mode="constant")
        return t[5:-5, 5:-5]

    for i in range(2):
        X, Y = x[i, 0].numpy(), y[i, 0].numpy()
        m1, m2 = filt(X), filt(Y)
        s1, s2, s12 = filt(X * X) - m1 * m1, filt(Y * Y) - m2 * m2, filt(X * Y) - m1 * m2
        want = (((2 * m1 * m2 + R.C1) / (m1 * m1 + m2 * m2 + R.C1)) * ((2 * s12 + R.C2) / (s1 + s2 + R.C2))).mean()
        assert abs(float(R.ssim_map(x[i:i + 1], y[i:i + 1]).mean()) - want) <= 1e-10


def test_taps_are_the_fp32_window_widened():
    t = R.taps()
    assert t.dtype == torch.float64 and torch.equal(t.float(), O.ssim_window(torch.float32)) and torch.equal(t, t.flip(0))


def test_kernel_source_holds_exactly_these_taps():
    """The kernel keeps the window as fp32 constants (libm's exp and a sequential sum give other last bits than torch, and 1e-7 in a tap
    is 1e-5 in the gradient): the constants in k_ssim_loss.hip are the oracle's window, bit for bit, and symmetric by construction."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m2trans_amd", "csrc", "k_ssim_loss.hip")).read()
    m = re.search(r"kTaps\[WIN / 2 \+ 1\] = \{([^}]*)\}", src)
    assert m, "the tap table of k_ssim_loss.hip was not found"
    vals = torch.tensor([float(v.strip().rstrip("f")) for v in m.group(1).split(",")], dtype=torch.float64).float()
    assert torch.equal(vals, O.ssim_window(torch.float32)[:6])


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_decide_sizes_and_bad_arguments_on_the_host():
    from m2trans_amd import _lib
    lib = _lib.load()
    assert lib.m2t_ssim_loss_scratch_bytes(2, 3, 10, 64) == 0 and lib.m2t_ssim_loss_scratch_bytes(2, 3, 64, 10) == 0
    assert lib.m2t_ssim_loss_scratch_bytes(1, 1, 11, 11) == 8
    assert lib.m2t_ssim_loss_scratch_bytes(2, 3, 75, 99) == 8 * 2 * 3 * 3 * 4            # one double per 32 x 32 tile and plane
    one = C.c_void_p(8)                                                                  # a non-null pointer that is never followed
    call = lambda **kw: lib.m2t_ssim_loss_tensor(*[kw.get(k, v) for k, v in (
        ("x", one), ("y", one), ("B", 1), ("C", 3), ("H", 16), ("W", 16), ("xs", 3 * 256), ("rs", 16), ("dr", 1.0), ("clamp", 1), ("scale", 1.0),
        ("gx", None), ("loss", one), ("acc", 0), ("scratch", one), ("stream", None))])
    for bad in (dict(x=None), dict(y=None), dict(loss=None), dict(scratch=None), dict(H=10), dict(W=10), dict(dr=0.0), dict(dr=-1.0),
                dict(dr=float("nan")), dict(dr=float("inf")), dict(rs=15), dict(xs=3 * 255), dict(xs=3 * 256 + 1), dict(B=0)):
        assert call(**bad) == -2, bad
    assert lib.m2t_ssim_loss(None, None, 1.0, 1.0, 1.0, None, 0, None, None, None) == -2


# ------------------------------------------------------------------------------------------------------------- TrainStep
def test_lambda_ssim_resolver_and_default():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep, resolve_lambda_ssim
    assert inspect.signature(TrainStep.__init__).parameters["lambda_ssim"].default == 0.0
    assert resolve_lambda_ssim(0) == 0.0 and resolve_lambda_ssim(0.1) == 0.1 and resolve_lambda_ssim("0.5") == 0.5
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), None, "much"):
        with pytest.raises(M2TError):
            resolve_lambda_ssim(bad)
    # the check comes before the model (None here) is looked at
    with pytest.raises(M2TError):
        TrainStep(None, lambda_ssim=-1.0)


def test_set_lambda_ssim_refuses_a_change_inside_an_accumulation_cycle():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    ts = TrainStep.__new__(TrainStep)
    ts.accum_steps, ts.micro_count, ts.ssim_loss, ts._ssim_scratch = 2, 1, None, {}
    with pytest.raises(M2TError):
        ts.set_lambda_ssim(0.0)
    ts.micro_count = 0
    ts.set_lambda_ssim(0.0)
    assert ts.lambda_ssim == 0.0 and ts.ssim_loss is None


# ------------------------------------------------------------------------------------------------------------- checkpoint
def _model():
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))


class _Step:
    """The flat-buffer part of TrainStep on the CPU, with the pixel loss and the weight of the structural term."""

    def __init__(self, m, pixel_loss="l1", pixel_loss_param=None, lambda_ssim=0.0, step_count=7, lr=5e-5):
        from m2trans_amd.train_step import TrainStep
        g = torch.Generator().manual_seed(step_count)
        self.exp_avg = torch.randn(m.flat_params.shape, generator=g)
        self.exp_avg_sq = torch.rand(m.flat_params.shape, generator=g)
        self.step_count, self.lr, self.scheduler_last_epoch = step_count, lr, 0
        self.micro_count, self.accum_steps = 0, 1
        TrainStep.set_pixel_loss(self, pixel_loss, pixel_loss_param)
        self.set_lambda_ssim(lambda_ssim)

    def set_pixel_loss(self, name, param=None):
        from m2trans_amd.train_step import TrainStep
        TrainStep.set_pixel_loss(self, name, param)

    def set_lambda_ssim(self, value):
        from m2trans_amd.train_step import resolve_lambda_ssim
        self.lambda_ssim = resolve_lambda_ssim(value)

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
    bare = types.SimpleNamespace(lr=5e-5, step_count=7, exp_avg=_Step(m).exp_avg, exp_avg_sq=_Step(m).exp_avg_sq)     # knows no lambda_ssim
    zero = export_checkpoint(m, _Step(m, lambda_ssim=0.0), epoch=3)
    assert list(zero) == keys and _same(zero, export_checkpoint(m, bare, epoch=3))
    # a non-L1 pixel term with lambda_ssim = 0: the entry of before, without the key
    assert export_checkpoint(m, _Step(m, "charbonnier", 1e-3), epoch=3)["m2t_loss"] == {"pixel_loss": "charbonnier", "param": 1e-3}


@pytest.mark.parametrize("name,param,entry", [("l1", None, {"pixel_loss": "l1", "param": None, "lambda_ssim": 0.1}),
                                              ("sl1", 0.25, {"pixel_loss": "smooth_l1", "param": 0.25, "lambda_ssim": 0.1})])
def test_checkpoint_entry_carries_lambda_ssim_and_round_trips(name, param, entry):
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model()
    src = _Step(m, name, param, lambda_ssim=0.1)
    ck = export_checkpoint(m, src, epoch=3)
    assert list(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict", "m2t_loss"]
    assert ck["m2t_loss"] == entry
    for start in (0.0, 0.7):                                                      # whatever the importing step was built with
        dst = _Step(_model(), "mse", None, lambda_ssim=start, step_count=1)
        assert import_checkpoint(ck, _model(), dst) == 4
        assert dst.lambda_ssim == 0.1 and (dst.pixel_loss, dst.pixel_loss_param) == (src.pixel_loss, src.pixel_loss_param)
        assert dst.step_count == 7 and torch.equal(dst.exp_avg, src.exp_avg)
    # a file whose entry has no lambda_ssim (saved with 0), and one without an entry, leave the importing step's weight alone
    dst = _Step(_model(), lambda_ssim=0.7)
    import_checkpoint(export_checkpoint(m, _Step(m, "mse"), epoch=3), _model(), dst)
    assert dst.lambda_ssim == 0.7 and dst.pixel_loss == "mse"
    import_checkpoint(export_checkpoint(m, _Step(m), epoch=3), _model(), dst)
    assert dst.lambda_ssim == 0.7
    # a plain object without the setters receives the attribute
    plain = types.SimpleNamespace(lr=1.0, step_count=0, exp_avg=torch.zeros_like(m.flat_params), exp_avg_sq=torch.zeros_like(m.flat_params),
                                  scheduler_last_epoch=0, set_lr=lambda lr: None)
    import_checkpoint(ck, _model(), plain)
    assert plain.lambda_ssim == 0.1


# ------------------------------------------------------------------------------------------------------------- host emulation
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"), shutil.which("clang++"), shutil.which("g++"))
                if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("ssim") / "ssim_emulate")
    subprocess.run([cxx, "-x", "c++", "-std=c++20", "-O2", "-ffp-contract=off", "-I", os.path.join(root, "tests", "emulate_hip"),
                    "-I", os.path.join(root, "m2trans_amd", "csrc"), os.path.join(root, "tests", "ssim_emulate.cpp"), "-o", exe, "-lpthread"],
                   check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("H,W,rs,clamp,phases", [(11, 11, 11, 0, (0.3, 0.7)), (12, 43, 43, 0, (0.3, 1.9)), (40, 56, 64, 1, (0.3, 1.9))],
                         ids=["one-entry", "two-row-map", "strided-clamp"])
def test_kernel_text_emulated_on_the_host_meets_the_gpu_gate(emulator, tmp_path, H, W, rs, clamp, phases):
    """csrc/m2t_ssim_tile.h on csrc/m2t_moment_tile.h -- the text the kernel runs, Tile<float, 32, 512> with the 1 - SSIM map, value then
    gradient -- on host threads (tests/ssim_emulate.cpp), the inputs of the GPU test's cases: one map entry; a two-row map, ragged; two
    tiles, clamp on, x in a NaN-filled buffer with a longer row.  The gradient within the gate of the GPU test's plan-free entry
    (1e-6 |ref| + 1e-7 scale + 6e-8 |prefill + ref|), the value within fp32 rounding (1e-6), nothing written outside [H, W]."""
    import struct
    import subprocess
    import numpy as np
    x = (O.closed_form_image(1, 1, H, W, phase=phases[0]) * 1.6 - 0.3).contiguous()
    y = O.closed_form_image(1, 1, H, W, phase=phases[1]).contiguous()
    if clamp:
        assert bool((x < 0).any()) and bool((x > 1).any())
    scale = 0.37 / ((H - 10) * (W - 10))
    want_loss, want = R.value_and_grad(x, y, 1.0, bool(clamp), scale)
    assert float(want.abs().max()) > 0
    g = torch.Generator().manual_seed(7)
    prefill = (torch.randn(H, rs, generator=g) * float(want.abs().max())).float()
    xb = torch.full((H, rs), float("nan"))
    xb[:, :W] = x[0, 0]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("4i", H, W, rs, clamp) + struct.pack("f", 1.0) + struct.pack("d", scale))
        f.write(xb.numpy().tobytes() + y[0, 0].numpy().tobytes() + prefill.numpy().tobytes())
    subprocess.run([emulator, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, capture_output=True)
    b = open(tmp_path / "out.bin", "rb").read()
    assert len(b) == 4 + 4 * H * rs
    loss = struct.unpack("f", b[:4])[0]
    gx = torch.from_numpy(np.frombuffer(b[4:], dtype=np.float32).copy()).view(H, rs)
    total = prefill[:, :W].double() + want[0, 0]
    bound = 1e-6 * want[0, 0].abs() + 1e-7 * scale + 6e-8 * total.abs()
    excess = float(((gx[:, :W].double() - total).abs() - bound).max())
    print(f"emulated tile {H}x{W}: largest excess over the gate {excess:.3e} (max |ref| {float(want.abs().max()):.3e}, scale {scale:.3e}); "
          f"value {loss:.9e} against {float(want_loss):.9e}")
    assert excess <= 0.0, excess
    if clamp:
        outside = (x[0, 0] < 0) | (x[0, 0] > 1)
        assert torch.equal(gx[:, :W][outside], prefill[:, :W][outside])                      # the clamp passes no gradient
    assert torch.equal(gx[:, W:].view(torch.int32), prefill[:, W:].view(torch.int32))
    assert abs(loss - float(want_loss)) <= 1e-6 * abs(float(want_loss))
