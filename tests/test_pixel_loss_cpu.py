"""CPU tests (no GPU) of TrainStep's pixel-loss family (l1, mse, charbonnier, smooth_l1): the fp64 restatement the GPU tests
compare the kernels with (tests/pixel_loss_ref.py) against torch's own loss modules and autograd, the C ABI table, TrainStep's
argument validation and the checkpoint entry."""
import ctypes as C
import inspect
import types

import pytest
import torch

from tests import pixel_loss_ref as R

BETA = 0.25


def _torch_loss(kind, param):
    if kind == "l1":
        return torch.nn.L1Loss()
    if kind == "mse":
        return torch.nn.MSELoss()
    if kind == "smooth_l1":
        return torch.nn.SmoothL1Loss(beta=param)
    # L1_Charbonnier_loss (reference losses.py:287-297)
    return lambda a, b: torch.mean(torch.sqrt((a - b) * (a - b) + param))


def _inputs():
    """fp64 (pre, hr) [2,3,8,12]: random values on both sides of the clamp, plus exact d = 0, |d| = beta, pre = 0 and pre = R."""
    g = torch.Generator().manual_seed(5)
    pre = torch.rand(2, 3, 8, 12, generator=g, dtype=torch.float64) * 1.6 - 0.3
    hr = torch.rand(2, 3, 8, 12, generator=g, dtype=torch.float64)
    pre[0, 0, 0, :8] = torch.tensor([0.5, 0.75, 0.25, 0.0, 1.0, 0.0, 1.0, 0.625], dtype=torch.float64)
    hr[0, 0, 0, :8] = torch.tensor([0.5, 0.5, 0.5, 0.25, 0.75, 0.0, 1.0, 0.625], dtype=torch.float64)
    d = pre.clamp(0, 1) - hr
    assert int((d == 0).sum()) >= 4 and int((d.abs() == BETA).sum()) >= 4
    assert int((pre == 0).sum()) >= 2 and int((pre == 1).sum()) >= 2 and int((pre < 0).sum()) > 10 and int((pre > 1).sum()) > 10
    return pre, hr


@pytest.mark.parametrize("kind,param", [("l1", None), ("mse", None), ("charbonnier", 1e-6), ("smooth_l1", BETA), ("smooth_l1", 1.0)])
def test_fp64_restatement_equals_torchs_losses_value_and_gradient(kind, param):
    pre, hr = _inputs()
    leaf = pre.clone().requires_grad_(True)
    want = _torch_loss(kind, param)(torch.clamp(leaf, 0.0, 1.0), hr)
    want.backward()
    want = want.detach()
    loss, seed = R.loss_and_seed(kind, pre, hr, param)
    assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want))
    assert float((seed - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max())
    # the clamp mask is inclusive (torch.clamp passes the gradient at pre = 0 and pre = R), the seed is 0 where the clamp is active
    assert bool((seed[(pre < 0) | (pre > 1)] == 0).all())
    if kind != "l1":
        on_edge = ((pre == 0) | (pre == 1)) & (pre != hr)
        assert int(on_edge.sum()) >= 2 and bool((seed[on_edge] != 0).all())


def test_fp64_restatement_default_parameters_and_padding():
    pre, hr = _inputs()
    assert float(R.loss_and_seed("charbonnier", pre, hr)[0]) == float(R.loss_and_seed("charbonnier", pre, hr, 1e-6)[0])
    assert float(R.loss_and_seed("smooth_l1", pre, hr)[0]) == float(R.loss_and_seed("smooth_l1", pre, hr, 1.0)[0])
    # a padded pre-clamp output: the padding carries no loss and no seed; weight / divisor scale both
    padded = torch.full((2, 3, 16, 16), 0.5, dtype=torch.float64)
    padded[..., :8, :12] = pre
    for kind in R.KINDS:
        l0, s0 = R.loss_and_seed(kind, pre, hr, BETA if kind == "smooth_l1" else None)
        l1, s1 = R.loss_and_seed(kind, padded, hr, BETA if kind == "smooth_l1" else None, weight=3.0, divisor=2 * hr.numel())
        assert abs(float(l1) - 1.5 * float(l0)) <= 1e-12 * abs(float(l0))
        assert float((s1[..., :8, :12] - 1.5 * s0).abs().max()) <= 1e-15
        assert int(torch.count_nonzero(s1[..., 8:, :])) == 0 and int(torch.count_nonzero(s1[..., :, 12:])) == 0


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Argument checks are decided on the host before anything touches a device."""
    from m2trans_amd import _lib
    lib = _lib.load()
    for fn in (lib.m2t_pixel_loss, lib.m2t_pixel_loss_deferred):
        assert fn(None, 0, 0.0, None, 1.0, 1.0, 1.0, None, None, None) == -2


def _bare_step():
    from m2trans_amd.train_step import TrainStep
    ts = TrainStep.__new__(TrainStep)
    ts.micro_count, ts.accum_steps = 0, 1
    return ts


def test_train_step_pixel_loss_names_aliases_and_defaults():
    from m2trans_amd.train_step import TrainStep, resolve_pixel_loss
    par = inspect.signature(TrainStep.__init__).parameters
    assert par["pixel_loss"].default == "l1" and par["pixel_loss_param"].default is None
    assert resolve_pixel_loss("l1") == (0, "l1", None)
    assert resolve_pixel_loss("mse") == resolve_pixel_loss("l2") == (1, "mse", None)
    assert resolve_pixel_loss("charbonnier") == (2, "charbonnier", 1e-6)
    assert resolve_pixel_loss("charbonnier", 1e-3) == (2, "charbonnier", 1e-3)
    assert resolve_pixel_loss("smooth_l1") == resolve_pixel_loss("sl1") == (3, "smooth_l1", 1.0)
    assert resolve_pixel_loss("sl1", BETA) == (3, "smooth_l1", BETA)
    ts = _bare_step()
    for name, param, want in [("l1", None, (0, "l1", None)), ("l2", None, (1, "mse", None)), ("sl1", BETA, (3, "smooth_l1", BETA)),
                              ("charbonnier", None, (2, "charbonnier", 1e-6))]:
        ts.set_pixel_loss(name, param)
        assert (ts._pixel_kind, ts.pixel_loss, ts.pixel_loss_param) == want


@pytest.mark.parametrize("name,param", [("huber", None), ("", None), (None, None), (2, None), ("l1", 1.0), ("mse", 0.5), ("charbonnier", 0.0),
                                        ("charbonnier", -1e-6), ("charbonnier", float("nan")), ("charbonnier", float("inf")),
                                        ("charbonnier", 1e-60), ("smooth_l1", 0.0), ("smooth_l1", -1.0), ("sl1", float("inf")),
                                        ("sl1", float("nan")), ("sl1", "wide")])
def test_train_step_refuses_unknown_names_and_bad_parameters_at_construction(name, param):
    """The check comes first in TrainStep.__init__: it raises before the model (None here) is looked at."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    with pytest.raises(M2TError) as e:
        TrainStep(None, pixel_loss=name, pixel_loss_param=param)
    if name in ("smooth_l1", "sl1") and param == 0.0:
        assert "l1" in str(e.value).replace("smooth_l1", "")          # beta = 0: the message names the l1 loss


def test_set_pixel_loss_refuses_a_change_inside_an_accumulation_cycle():
    from m2trans_amd._lib import M2TError
    ts = _bare_step()
    ts.accum_steps, ts.micro_count = 2, 1
    with pytest.raises(M2TError):
        ts.set_pixel_loss("mse")


# ------------------------------------------------------------------------------------------------------------- checkpoint
def _model():
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))


class _Step:
    """The flat-buffer part of TrainStep on the CPU, with the pixel loss."""

    def __init__(self, m, pixel_loss="l1", pixel_loss_param=None, step_count=7, lr=5e-5):
        from m2trans_amd.train_step import TrainStep
        g = torch.Generator().manual_seed(step_count)
        self.exp_avg = torch.randn(m.flat_params.shape, generator=g)
        self.exp_avg_sq = torch.rand(m.flat_params.shape, generator=g)
        self.step_count, self.lr, self.scheduler_last_epoch = step_count, lr, 0
        self.micro_count, self.accum_steps = 0, 1
        TrainStep.set_pixel_loss(self, pixel_loss, pixel_loss_param)

    def set_pixel_loss(self, name, param=None):
        from m2trans_amd.train_step import TrainStep
        TrainStep.set_pixel_loss(self, name, param)

    def set_lr(self, lr):
        self.lr = lr


def test_checkpoint_of_an_l1_step_carries_no_loss_entry():
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model()
    bare = types.SimpleNamespace(lr=5e-5, step_count=7, exp_avg=torch.randn_like(m.flat_params), exp_avg_sq=torch.rand_like(m.flat_params))
    keys = ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict"]
    assert list(export_checkpoint(m, bare, epoch=3)) == keys                      # an object that knows no pixel losses
    ck = export_checkpoint(m, _Step(m), epoch=3)
    assert list(ck) == keys
    # a file without the entry leaves the importing step's loss alone
    dst = _Step(_model(), "smooth_l1", BETA)
    assert import_checkpoint(ck, _model(), dst) == 4
    assert (dst._pixel_kind, dst.pixel_loss, dst.pixel_loss_param) == (3, "smooth_l1", BETA)


@pytest.mark.parametrize("name,param,entry", [("mse", None, {"pixel_loss": "mse", "param": None}),
                                              ("l2", None, {"pixel_loss": "mse", "param": None}),
                                              ("charbonnier", None, {"pixel_loss": "charbonnier", "param": 1e-6}),
                                              ("charbonnier", 1e-4, {"pixel_loss": "charbonnier", "param": 1e-4}),
                                              ("smooth_l1", None, {"pixel_loss": "smooth_l1", "param": 1.0}),
                                              ("sl1", BETA, {"pixel_loss": "smooth_l1", "param": BETA})])
def test_checkpoint_loss_entry_round_trips(name, param, entry):
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model()
    src = _Step(m, name, param)
    ck = export_checkpoint(m, src, epoch=3)
    assert list(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict", "m2t_loss"]
    assert ck["m2t_loss"] == entry
    for start in ("l1", "charbonnier"):                                           # whatever the importing step was built with
        dst = _Step(_model(), start, step_count=99)
        assert import_checkpoint(ck, _model(), dst) == 4
        assert (dst._pixel_kind, dst.pixel_loss, dst.pixel_loss_param) == (src._pixel_kind, src.pixel_loss, src.pixel_loss_param)
        assert dst.step_count == 7 and torch.equal(dst.exp_avg, src.exp_avg)
    # a plain object without set_pixel_loss receives the two attributes
    plain = types.SimpleNamespace(lr=1.0, step_count=0, exp_avg=torch.zeros_like(m.flat_params), exp_avg_sq=torch.zeros_like(m.flat_params),
                                  scheduler_last_epoch=0, set_lr=lambda lr: None)
    import_checkpoint(ck, _model(), plain)
    assert (plain.pixel_loss, plain.pixel_loss_param) == (entry["pixel_loss"], entry["param"])
