"""CPU tests (no GPU) of the MS-SSIM loss term (TrainStep(lambda_msssim=...), m2t_msssim_loss / m2t_msssim_loss_tensor): the fp64
restatement the GPU tests compare the kernels with (tests/msssim_loss_ref.py) -- its analytic gradient against torch autograd, its
pooling against F.avg_pool2d and an index loop, the identity and the zero rule -- the C ABI table of include/m2t_msssim.h,
TrainStep's argument validation and the checkpoint entry."""
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from tests import msssim_loss_ref as R
from tests import ssim_loss_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape,sigma", [((1, 2, 161, 161), 0.02), ((1, 1, 177, 200), 0.3)], ids=["odd-chain", "mixed-parity"])
def test_analytic_gradient_equals_autograd_of_the_restatement_in_fp64(shape, sigma):
    """The two-phase gradient (level coefficients w_l M / (v_l n_l), the cs coefficient maps, the pooling adjoint) against autograd of
    ms_ssim: the difference is rounding, <= 1e-10 of the largest entry."""
    x, y = R.smooth_pair(shape, sigma, seed=1)
    x, y = x.double(), y.double()
    assert float(R.level_values(x, y).min()) > 0
    leaf = x.clone().requires_grad_(True)
    M = R.ms_ssim(leaf, y)
    (1.0 - M).sum().backward()
    value, grad, Mv, levels = R.value_and_grad(x, y)
    assert torch.equal(Mv, M.detach()) and float(value) == float((1.0 - M.detach()).sum())
    assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    err = float((grad - leaf.grad).abs().max() / leaf.grad.abs().max())
    print(f"{shape} sigma {sigma}: analytic against autograd, {err:.3e} of the largest entry; min v {float(R.level_values(x, y).min()):.3f}")
    assert err <= 1e-10, err
    assert [tuple(t.shape[-2:]) for t in levels] == [tuple(t.shape[-2:]) for t in R.pyramid(x)[1:]]


def test_loss_and_seed_equals_autograd_through_the_clamp_and_the_padded_layout():
    Rr, w = 2.0, 0.3
    x, y = R.smooth_pair((1, 3, 162, 170), 0.05, seed=2, R=Rr, spill=True)
    x = x.double()                                                      # (a tenth of the values outside [0, R])
    pre = torch.zeros(1, 3, 192, 192, dtype=torch.float64)
    pre[..., :162, :170] = x
    pre[..., 162:, :] = 7.0                                             # the padding is never read
    inner = pre[..., :162, :170]
    share = float(((inner < 0) | (inner > Rr)).double().mean())
    assert 0.05 < share < 0.2, share
    assert float(R.level_values(inner.clamp(0.0, Rr) / Rr, y.double() / Rr).min()) > 0
    leaf = pre.clone().requires_grad_(True)
    M = R.ms_ssim(leaf[..., :162, :170].clamp(0.0, Rr) / Rr, y.double() / Rr)
    want = w * (1.0 - M).sum() / 12.0
    want.backward()
    loss, seed = R.loss_and_seed(pre, y, weight=w, divisor=12.0, R=Rr)
    assert abs(float(loss) - float(want.detach())) <= 1e-14
    assert float((seed - leaf.grad).abs().max()) <= 1e-10 * float(leaf.grad.abs().max())
    assert int(torch.count_nonzero(seed[..., 162:, :])) == 0 and int(torch.count_nonzero(seed[..., :, 170:])) == 0
    assert int(torch.count_nonzero(seed[..., :162, :170][(inner < 0) | (inner > Rr)])) == 0
    assert float(R.loss_and_seed(pre, y, R=Rr)[0]) == pytest.approx(float(want.detach()) * 12.0 / 3.0 / w, rel=1e-13)   # default: the mean


@pytest.mark.parametrize("H,W", [(5, 7), (6, 6), (6, 5)])
def test_pooling_rule_matches_an_index_loop_and_avg_pool2d(H, W):
    g = torch.Generator().manual_seed(H * 10 + W)
    t = torch.rand(2, H, W, generator=g, dtype=torch.float64)
    got = R.pool(t)
    Ho, Wo = H // 2 + H % 2, W // 2 + W % 2
    assert tuple(got.shape) == (2, Ho, Wo) and R.pooled_side(H) == Ho
    want = torch.zeros(2, Ho, Wo, dtype=torch.float64)
    for i in range(Ho):
        for j in range(Wo):
            for di in range(2):
                for dj in range(2):
                    a, b = 2 * i - H % 2 + di, 2 * j - W % 2 + dj      # with an odd side the cells start at index -1
                    if 0 <= a < H and 0 <= b < W:
                        want[:, i, j] += t[:, a, b]
    want *= 0.25
    assert float((got - want).abs().max()) <= 1e-15
    ref = F.avg_pool2d(t[None], kernel_size=2, stride=2, padding=(H % 2, W % 2))[0]       # count_include_pad=True: zeros counted
    assert float((got - ref).abs().max()) <= 1e-15
    # the adjoint: <pool(t), g> == <t, pool_t(g)>
    gg = torch.rand(2, Ho, Wo, generator=g, dtype=torch.float64)
    assert abs(float((got * gg).sum() - (t * R.pool_t(gg, H, W)).sum())) <= 1e-13


def test_identity_gives_one_and_no_gradient():
    _, y = R.smooth_pair((1, 2, 161, 176), 0.0, seed=3)
    value, grad, M, _ = R.value_and_grad(y, y)
    assert float((M - 1.0).abs().max()) <= 1e-12 and abs(float(value)) <= 1e-12
    assert float(grad.abs().max()) <= 1e-9                          # rounding level: every map is flat at its maximum


def test_zero_rule_on_the_inverted_image():
    """x = 1 - y at 176 x 176: the first four level means are negative, M = 0, the gradient is exactly 0 (autograd gives NaN)."""
    _, y = R.smooth_pair((1, 2, 176, 176), 0.0, seed=4)
    x = 1.0 - y
    v = R.level_values(x.double(), y.double())
    assert bool((v[..., :4] < 0).all()), v
    value, grad, M, levels = R.value_and_grad(x, y, scale=0.5)
    assert int(torch.count_nonzero(M)) == 0 and float(value) == 0.5 * 2
    assert int(torch.count_nonzero(grad)) == 0 and all(int(torch.count_nonzero(t)) == 0 for t in levels)
    assert float(R.ms_ssim(x.double(), y.double()).abs().max()) == 0.0
    # one dead and one live channel in the same call
    xm = torch.cat([x[:, :1], y[:, 1:] * 0.9], dim=1)
    value, grad, M, _ = R.value_and_grad(xm, y)
    assert float(M[0, 0]) == 0.0 and 0.0 < float(M[0, 1]) < 1.0
    assert int(torch.count_nonzero(grad[:, 0])) == 0 and float(grad[:, 1].abs().max()) > 0


def test_weights_and_size_rule():
    from m2trans_amd import _lib
    from m2trans_amd.train_step import msssim_size_supported
    assert R.WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) == _lib.MSSSIM_WEIGHTS and R.LEVELS == 5
    assert abs(sum(R.WEIGHTS) - 1.0001) < 1e-12                     # (the packages' weights do not sum to exactly 1)
    assert R.MIN_SIDE == 161 == _lib.MSSSIM_MIN_SIDE
    assert msssim_size_supported(161, 161) and not msssim_size_supported(160, 400) and not msssim_size_supported(400, 160)
    n = 161
    for _ in range(4):
        n = R.pooled_side(n)
    assert n == S.WIN                                               # level 4 of the smallest side holds exactly one window
    src = open(os.path.join(ROOT, "m2trans_amd", "csrc", "k_msssim_loss.hip")).read()
    m = re.search(r"w\[LEVELS\] = \{([^}]*)\}", src)
    assert m and tuple(float(t) for t in m.group(1).split(",")) == R.WEIGHTS


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_decide_sizes_and_bad_arguments_on_the_host():
    from m2trans_amd import _lib
    lib = _lib.load()
    bad_off = C.c_size_t(-1).value
    assert lib.m2t_msssim_loss_scratch_bytes(2, 3, 160, 400) == 0 and lib.m2t_msssim_loss_scratch_bytes(2, 3, 400, 160) == 0
    assert lib.m2t_msssim_loss_scratch_bytes(0, 3, 200, 200) == 0 and lib.m2t_msssim_loss_scratch_bytes(21846, 3, 200, 200) == 0
    # 161 x 161, one plane: record 12; tiles 36 + 36 + 9 + 4 + 1; three sets of levels 81^2 + 41^2 + 21^2 + 11^2
    levels = 81 * 81 + 41 * 41 + 21 * 21 + 11 * 11
    assert lib.m2t_msssim_loss_scratch_bytes(1, 1, 161, 161) == 8 * (12 + 36 + 36 + 9 + 4 + 1 + 3 * levels)
    assert lib.m2t_msssim_loss_scratch_offset(1, 1, 161, 161, 0, 0) == 0
    assert lib.m2t_msssim_loss_scratch_offset(1, 1, 161, 161, 1, 0) == 8 * 12
    assert lib.m2t_msssim_loss_scratch_offset(1, 1, 161, 161, 2, 1) == 8 * (12 + 86)
    assert lib.m2t_msssim_loss_scratch_offset(1, 1, 161, 161, 3, 1) == 8 * (12 + 86 + levels)
    assert lib.m2t_msssim_loss_scratch_offset(1, 1, 161, 161, 4, 4) == 8 * (12 + 86 + 3 * levels - 121)
    for bad in ((1, 1, 160, 161, 0, 0), (1, 1, 161, 161, 2, 0), (1, 1, 161, 161, 5, 1), (1, 1, 161, 161, 1, 5), (1, 1, 161, 161, 1, -1)):
        assert lib.m2t_msssim_loss_scratch_offset(*bad) == bad_off, bad
    one = C.c_void_p(8)                                              # a non-null pointer that is never followed
    call = lambda **kw: lib.m2t_msssim_loss_tensor(*[kw.get(k, v) for k, v in (
        ("x", one), ("y", one), ("B", 1), ("C", 3), ("H", 176), ("W", 192), ("xs", 3 * 176 * 192), ("rs", 192), ("dr", 1.0), ("clamp", 1),
        ("scale", 1.0), ("gx", None), ("loss", one), ("per", None), ("acc", 0), ("scratch", one), ("stream", None))])
    for bad in (dict(x=None), dict(y=None), dict(loss=None), dict(scratch=None), dict(H=160), dict(W=160), dict(H=10), dict(dr=0.0),
                dict(dr=-1.0), dict(dr=float("nan")), dict(dr=float("inf")), dict(rs=191), dict(xs=3 * 176 * 192 - 3),
                dict(xs=3 * 176 * 192 + 1), dict(B=0), dict(B=21846)):
        assert call(**bad) == -2, bad
    assert call(H=160) == -2 and b"larger than 160" in lib.m2t_last_error_string()
    assert lib.m2t_msssim_loss(None, None, 1.0, 1.0, 1.0, None, 0, None, None, None) == -2


def test_python_entries_refuse_host_tensors_and_small_images():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import MSSSIMLoss, ms_ssim_loss
    from m2trans_amd.metrics import ms_ssim_device
    x = torch.zeros(1, 3, 176, 176)
    for fn in (ms_ssim_loss, ms_ssim_device, MSSSIMLoss()):
        with pytest.raises(M2TError):
            fn(x, x)                                                 # host tensors: no fallback
        with pytest.raises(M2TError):
            fn(x, x[..., :160])
    with pytest.raises(M2TError):
        ms_ssim_loss(x, x, data_range=0.0)


# ------------------------------------------------------------------------------------------------------------- TrainStep
def test_lambda_msssim_resolver_and_default():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep, resolve_lambda_msssim
    assert inspect.signature(TrainStep.__init__).parameters["lambda_msssim"].default == 0.0
    assert resolve_lambda_msssim(0) == 0.0 and resolve_lambda_msssim(0.16) == 0.16 and resolve_lambda_msssim("0.5") == 0.5
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), None, "much"):
        with pytest.raises(M2TError):
            resolve_lambda_msssim(bad)
    # the check comes before the model (None here) is looked at
    with pytest.raises(M2TError):
        TrainStep(None, lambda_msssim=-1.0)


def test_set_lambda_msssim_refuses_a_change_inside_an_accumulation_cycle():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    ts = TrainStep.__new__(TrainStep)
    ts.accum_steps, ts.micro_count, ts.msssim_loss, ts._msssim_scratch = 2, 1, None, {}
    with pytest.raises(M2TError):
        ts.set_lambda_msssim(0.0)
    ts.micro_count = 0
    ts.set_lambda_msssim(0.0)
    assert ts.lambda_msssim == 0.0 and ts.msssim_loss is None and ts._msssim_scratch == {}


def test_size_is_refused_before_any_launch():
    """_scratch_for refuses a small SR image on the host: no library call is made (lib = None would raise otherwise)."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import _TERM, TrainStep
    ts = TrainStep.__new__(TrainStep)
    ts._msssim_scratch = {}
    with pytest.raises(M2TError, match="larger than 160"):
        ts._scratch_for(_TERM["msssim"], None, torch.zeros(2, 3, 160, 224))


# ------------------------------------------------------------------------------------------------------------- checkpoint
def _model():
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))


class _Step:
    """The flat-buffer part of TrainStep on the CPU, with the pixel loss and the weights of the structural terms."""

    def __init__(self, m, pixel_loss="l1", pixel_loss_param=None, lambda_msssim=0.0, lambda_ssim=0.0, step_count=7, lr=5e-5):
        from m2trans_amd.train_step import TrainStep
        g = torch.Generator().manual_seed(step_count)
        self.exp_avg = torch.randn(m.flat_params.shape, generator=g)
        self.exp_avg_sq = torch.rand(m.flat_params.shape, generator=g)
        self.step_count, self.lr, self.scheduler_last_epoch = step_count, lr, 0
        self.micro_count, self.accum_steps = 0, 1
        self.lambda_ssim = lambda_ssim
        TrainStep.set_pixel_loss(self, pixel_loss, pixel_loss_param)
        self.set_lambda_msssim(lambda_msssim)

    def set_pixel_loss(self, name, param=None):
        from m2trans_amd.train_step import TrainStep
        TrainStep.set_pixel_loss(self, name, param)

    def set_lambda_ssim(self, value):
        self.lambda_ssim = float(value)

    def set_lambda_msssim(self, value):
        from m2trans_amd.train_step import resolve_lambda_msssim
        self.lambda_msssim = resolve_lambda_msssim(value)

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
    bare = types.SimpleNamespace(lr=5e-5, step_count=7, exp_avg=_Step(m).exp_avg, exp_avg_sq=_Step(m).exp_avg_sq)     # knows no lambda_msssim
    zero = export_checkpoint(m, _Step(m, lambda_msssim=0.0), epoch=3)
    assert list(zero) == keys and _same(zero, export_checkpoint(m, bare, epoch=3))
    # the other terms with lambda_msssim = 0: the entries of before, without the key
    assert export_checkpoint(m, _Step(m, "charbonnier", 1e-3), epoch=3)["m2t_loss"] == {"pixel_loss": "charbonnier", "param": 1e-3}
    assert export_checkpoint(m, _Step(m, lambda_ssim=0.1), epoch=3)["m2t_loss"] == {"pixel_loss": "l1", "param": None, "lambda_ssim": 0.1}


@pytest.mark.parametrize("name,param,entry", [("l1", None, {"pixel_loss": "l1", "param": None, "lambda_msssim": 0.16}),
                                              ("sl1", 0.25, {"pixel_loss": "smooth_l1", "param": 0.25, "lambda_msssim": 0.16})])
def test_checkpoint_entry_carries_lambda_msssim_and_round_trips(name, param, entry):
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model()
    src = _Step(m, name, param, lambda_msssim=0.16)
    ck = export_checkpoint(m, src, epoch=3)
    assert list(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict", "m2t_loss"]
    assert ck["m2t_loss"] == entry
    for start in (0.0, 0.7):                                                      # whatever the importing step was built with
        dst = _Step(_model(), "mse", None, lambda_msssim=start, step_count=1)
        assert import_checkpoint(ck, _model(), dst) == 4
        assert dst.lambda_msssim == 0.16 and (dst.pixel_loss, dst.pixel_loss_param) == (src.pixel_loss, src.pixel_loss_param)
        assert dst.step_count == 7 and torch.equal(dst.exp_avg, src.exp_avg)
    # a file whose entry has no lambda_msssim (saved with 0), and one without an entry, leave the importing step's weight alone
    dst = _Step(_model(), lambda_msssim=0.7)
    import_checkpoint(export_checkpoint(m, _Step(m, "mse"), epoch=3), _model(), dst)
    assert dst.lambda_msssim == 0.7 and dst.pixel_loss == "mse"
    import_checkpoint(export_checkpoint(m, _Step(m), epoch=3), _model(), dst)
    assert dst.lambda_msssim == 0.7
    # with the SSIM term next to it: both keys, in the order SSIM, MS-SSIM
    both = export_checkpoint(m, _Step(m, lambda_msssim=0.16, lambda_ssim=0.1), epoch=3)["m2t_loss"]
    assert list(both) == ["pixel_loss", "param", "lambda_ssim", "lambda_msssim"]
    # a plain object without the setters receives the attribute
    plain = types.SimpleNamespace(lr=1.0, step_count=0, exp_avg=torch.zeros_like(m.flat_params), exp_avg_sq=torch.zeros_like(m.flat_params),
                                  scheduler_last_epoch=0, set_lr=lambda lr: None)
    import_checkpoint(ck, _model(), plain)
    assert plain.lambda_msssim == 0.16


# ------------------------------------------------------------------------------------------------------------- host emulation
def test_tile_text_emulated_on_the_host_meets_the_gpu_gate(tmp_path):
    """csrc/m2t_ssim_tile.h -- the text both structural kernels run -- on host threads (tests/msssim_emulate.cpp) at 161 x 161, every
    level odd, R = 255, clamp on, x in a buffer with a longer row: the pyramid bit for bit, the gradient within the gate of the GPU
    test (1e-6 |ref| + 1e-7 max |ref| + 6e-8 |prefill + ref|), the value 1e-6, M 1e-12, nothing written outside [H, W]."""
    import shutil
    import struct
    import subprocess
    import numpy as np
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"), shutil.which("clang++"), shutil.which("g++"))
                if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path / "msssim_emulate")
    subprocess.run([cxx, "-x", "c++", "-std=c++20", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "emulate_hip"),
                    "-I", os.path.join(ROOT, "m2trans_amd", "csrc"), os.path.join(ROOT, "tests", "msssim_emulate.cpp"), "-o", exe, "-lpthread"],
                   check=True, capture_output=True)
    H, W, rs, Rr, scale = 161, 161, 168, 255.0, 0.37
    x, y = R.smooth_pair((1, 1, H, W), 0.02, seed=10, R=Rr, spill=True)
    want_loss, want, want_M, _ = R.value_and_grad(x, y, Rr, True, scale)
    assert float(want_M) > 0
    g = torch.Generator().manual_seed(7)
    prefill = (torch.randn(H, rs, generator=g) * float(want.abs().max())).float()
    xb = torch.full((H, rs), float("nan"))
    xb[:, :W] = x[0, 0]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("4i", H, W, rs, 1) + struct.pack("f", Rr) + struct.pack("d", scale))
        f.write(xb.numpy().tobytes() + y[0, 0].numpy().tobytes() + prefill.numpy().tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, capture_output=True)
    b = open(tmp_path / "out.bin", "rb").read()
    loss, M = struct.unpack("f", b[:4])[0], struct.unpack("d", b[4:12])[0]
    gx = torch.from_numpy(np.frombuffer(b[12:12 + 4 * H * rs], dtype=np.float32).copy()).view(H, rs)
    off = 12 + 4 * H * rs
    for level in R.pyramid(x.double().clamp(0.0, Rr))[1:]:
        got = torch.from_numpy(np.frombuffer(b[off:off + 8 * level.numel()], dtype=np.float64).copy())
        off += 8 * level.numel()
        assert torch.equal(got.view(torch.int64), level.flatten().contiguous().view(torch.int64)), tuple(level.shape)
    total = prefill[:, :W].double() + want[0, 0]
    bound = 1e-6 * want[0, 0].abs() + 1e-7 * want.abs().max() + 6e-8 * total.abs()
    ratio = float(((gx[:, :W].double() - total).abs() / bound).max())
    print(f"emulated tile: largest |got - ref| / bound {ratio:.3f}; value {loss:.9e} against {float(want_loss):.9e}; M {M:.15f}")
    assert ratio <= 1.0, ratio
    assert torch.equal(gx[:, W:].view(torch.int32), prefill[:, W:].view(torch.int32))
    assert abs(loss - float(want_loss)) <= 1e-6 * float(want_loss) and abs(M - float(want_M)) <= 1e-12 * float(want_M)
