"""The optional loss terms of TrainStep as ONE sequence (train_step.LOSS_TERMS, then the perceptual term), on the host against a
recording stand-in for the library: every on/off subset of the five terms issues the calls in the fixed order behind one pixel entry,
every size / scratch query comes before m2t_forward, an accumulation cycle stores in its first micro-batch and adds in the others with
the table's count times accum_steps as the divisor, the differentiable-SemanticLoss route issues the same sequence, and a checkpoint
carries all five weights and their settings in the fixed key order.  No device is needed."""
import contextlib
import itertools
import types

import pytest
import torch

TERMS = ("ssim", "msssim", "fft", "vif", "perceptual")                       # the fixed order
ENTRY = {"ssim": "m2t_ssim_loss", "msssim": "m2t_msssim_loss", "fft": "m2t_fft_loss", "vif": "m2t_vif_loss", "perceptual": "m2t_vgg_loss"}
LAM = {"ssim": 0.1, "msssim": 0.16, "fft": 0.2, "vif": 0.05, "perceptual": 0.03}
B, HS, WS = 2, 192, 192
# what each term's mean runs over for one (2, 3, 192, 192) micro-batch, and where its C call carries (weight, divisor, store / add)
COUNT = {"ssim": B * 3 * (HS - 10) * (WS - 10), "msssim": B * 3, "fft": B * 3 * HS * (WS // 2 + 1) * 2, "vif": B, "perceptual": B}
ARGS = {"ssim": (2, 3, 6), "msssim": (2, 3, 6), "fft": (2, 3, 7), "vif": (2, 3, 7), "perceptual": (3, 4, 10)}
SUBSETS = [tuple(t for t, on in zip(TERMS, bits) if on) for bits in itertools.product((False, True), repeat=len(TERMS))]


class _Calls:
    """A stand-in for the loaded library: records (entry point, arguments) in call order, every call succeeds."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def fn(*a):
            self.log.append((name, a))
            return 1 << 20 if name.endswith("_bytes") else 0
        return fn

    @property
    def names(self):
        return [n for n, _ in self.log]

    def launches(self):
        """The recorded names without the size / scratch / workspace queries."""
        return [n for n in self.names if not n.endswith("_bytes")]


def _tower(calls, **kw):
    """A stand-in for losses.PerceptualLoss with weights loaded; its workspace query is recorded next to the library's."""
    def workspace(b, h, w, want_grad):
        calls.log.append(("m2t_vgg_workspace_bytes", (b, h, w, want_grad)))
        return None
    d = dict(loaded=True, resize=False, data_range=1.0, criterion="sl1", weights=[1.0, 0.5, 0.0, 2.0, 1.5], kind=3, param=1.0, handle="H",
             tap_weights=lambda: "TW", workspace=workspace)
    d.update(kw)
    return types.SimpleNamespace(**d)


class _Semantic:
    """A differentiable SemanticLoss as far as TrainStep looks at it: a value, a dense gradient, no crop origins."""
    differentiable = True

    def _value_and_grad(self, sr, hr, captions):
        return torch.ones(1), torch.zeros_like(sr), None


def _host_step(monkeypatch, on, accum_steps=1, semantic=False):
    """A step object assembled without __init__ (it starts from the class defaults), the terms of `on` switched on by their setters."""
    from m2trans_amd import _lib, train_step as T
    calls = _Calls()
    monkeypatch.setattr(_lib, "load", lambda: calls)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(_lib, "ptr", lambda t: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    plan = types.SimpleNamespace(handle=None, workspace=None, gen=0, trained=False)
    model = types.SimpleNamespace(scale=2, rgb_range=1.0, flat_params=torch.zeros(4), _plan_for=lambda lr: plan)
    ts = T.TrainStep.__new__(T.TrainStep)
    ts.model, ts.micro_count, ts.accum_steps, ts.world_size = model, 0, accum_steps, 1
    ts.semantic_loss, ts.lambda_clip, ts.lambda_l1 = (_Semantic(), 0.5, 1.0) if semantic else (None, 0.0, 1.0)
    ts.grads, ts.l1_loss = torch.zeros(4), torch.zeros(1)
    ts.micro_grads, ts.micro_loss = (torch.zeros(4), torch.zeros(1)) if accum_steps > 1 else (None, None)
    ts.set_pixel_loss("l1", None)
    ts.perceptual_loss = _tower(calls)
    for t in on:
        getattr(ts, f"set_lambda_{t}")(LAM[t])
    return ts, calls


def _micro_batch(ts, captions=None):
    return ts.forward_backward(torch.zeros(B, 3, HS // 2, WS // 2), torch.zeros(B, 3, HS, WS), captions)


@pytest.mark.parametrize("on", SUBSETS, ids=["+".join(s) or "none" for s in SUBSETS])
def test_every_subset_issues_the_fixed_sequence_and_asks_for_scratch_before_the_forward(monkeypatch, on):
    ts, calls = _host_step(monkeypatch, on)
    loss = _micro_batch(ts)
    pixel = "m2t_l1_loss" if on else "m2t_l1_loss_deferred"                  # deferred iff no optional term is on
    assert calls.launches() == ["m2t_forward", pixel] + [ENTRY[t] for t in on] + ["m2t_backward"]
    forward = calls.names.index("m2t_forward")
    scratch = [i for i, n in enumerate(calls.names) if n.endswith("scratch_bytes")]
    assert len(scratch) == len(set(on) - {"perceptual"}) and all(i < forward for i in scratch)
    if "perceptual" in on:                                                   # (the tower caches its workspace; the call looks it up again)
        assert calls.names.index("m2t_vgg_workspace_bytes") < forward
    # the total is the pixel value plus the values of the terms that are on (all zeros here: the shapes and the identity are the check)
    assert loss is ts.loss and (loss is ts.l1_loss) == (not on) and loss.shape == (1,)
    for t in TERMS:
        value = ts.perceptual_loss_value if t == "perceptual" else getattr(ts, f"{t}_loss")
        assert (value is not None) == (t in on), t


def test_an_accumulation_cycle_stores_then_adds_and_divides_by_the_table_count_times_accum_steps(monkeypatch):
    ts, calls = _host_step(monkeypatch, TERMS, accum_steps=2)
    _micro_batch(ts)
    split = len(calls.log)
    _micro_batch(ts)
    sequence = ["m2t_forward", "m2t_l1_loss"] + [ENTRY[t] for t in TERMS] + ["m2t_backward"]
    first, second = calls.log[:split], calls.log[split:]
    assert [n for n, _ in first if not n.endswith("_bytes")] == sequence
    assert [n for n, _ in second if not n.endswith("_bytes")] == sequence + ["m2t_grad_accumulate"]
    for micro, flag in ((first, 0), (second, 1)):
        got = dict(micro)
        for t in TERMS:
            w, d, acc = ARGS[t]
            a = got[ENTRY[t]]
            assert a[w] == LAM[t] and a[d] == float(COUNT[t] * 2) and a[acc] == flag, (t, flag)
    assert dict(first)["m2t_fft_loss"][5] == 0 and dict(first)["m2t_vif_loss"][5] == 2.0        # norm 'backward', sigma_n_sq
    # the scratch of a shape is asked for once per step object, not once per micro-batch
    assert not [n for n, _ in second if n.endswith("scratch_bytes")]


def test_the_differentiable_semantic_route_issues_the_same_sequence(monkeypatch):
    for on in ((), ("ssim", "vif"), TERMS):
        ts, calls = _host_step(monkeypatch, on, semantic=True)
        _micro_batch(ts, captions=["a", "b"])
        assert calls.launches() == ["m2t_forward", "m2t_l1_loss"] + [ENTRY[t] for t in on] + ["m2t_add_output_grad", "m2t_backward"], on
        assert all(dict(calls.log)[ENTRY[t]][ARGS[t][2]] == 0 for t in on)


def test_a_size_a_term_does_not_take_is_refused_before_any_launch(monkeypatch):
    """SSIM included: its refusal used to come after m2t_forward and the pixel loss had been enqueued."""
    from m2trans_amd._lib import M2TError
    ts, calls = _host_step(monkeypatch, ("ssim",))
    monkeypatch.setattr(ts.model, "scale", 1)
    with pytest.raises(M2TError, match="lambda_ssim > 0: the SR image 10x64 is smaller than the 11 x 11 SSIM window"):
        ts.forward_backward(torch.zeros(B, 3, 10, 64), torch.zeros(B, 3, 10, 64))
    assert calls.names == []


def test_class_defaults_are_off_for_every_term_and_scratch_caches_are_per_object():
    from m2trans_amd.train_step import _TERM, LOSS_TERMS, TrainStep
    # the single table, in call order
    assert [t.name for t in LOSS_TERMS] == ["ssim", "msssim", "fft", "vif", "gmsd", "wavelet", "consistency"]
    a, b = TrainStep.__new__(TrainStep), TrainStep.__new__(TrainStep)
    for t in TERMS[:4]:
        assert getattr(a, f"lambda_{t}") == 0.0 and getattr(a, f"{t}_loss") is None and getattr(a, f"_{t}_scratch") is None
    assert a.lambda_perceptual == 0.0 and a.perceptual_loss is None and a.perceptual_loss_value is None and a.fft_norm == "backward"
    lib = types.SimpleNamespace(m2t_vif_loss_scratch_bytes=lambda *s: 64)
    a._scratch_for(_TERM["vif"], lib, torch.zeros(1, 3, 48, 48))
    assert list(a._vif_scratch) == [(1, 48, 48)] and b._vif_scratch is None and TrainStep._vif_scratch is None


def test_resolve_lambda_names_the_term_in_the_one_message():
    from m2trans_amd import train_step as T
    from m2trans_amd._lib import M2TError
    for t in TERMS:
        bound = getattr(T, f"resolve_lambda_{t}")
        assert bound(0) == 0.0 and bound("0.5") == 0.5 == T.resolve_lambda(t, 0.5)
        for bad in (-0.1, float("nan"), float("inf"), None, "much"):
            with pytest.raises(M2TError) as e:
                bound(bad)
            assert str(e.value) == f"lambda_{t} must be a finite number >= 0, got {bad!r}"


def test_checkpoint_round_trip_of_all_five_terms(monkeypatch):
    from m2trans_amd import train_step as T
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    from m2trans_amd.M2Trans_network import create_model
    model = lambda: create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))

    def step(m, on):
        ts, calls = _host_step(monkeypatch, ())
        ts.model = m
        ts.perceptual_loss.configure = lambda w, c, r: ts.perceptual_loss.__dict__.update(weights=list(w), criterion=c, resize=r)
        ts.exp_avg, ts.exp_avg_sq = torch.ones_like(m.flat_params), torch.ones_like(m.flat_params)
        ts.step_count, ts.lr, ts.scheduler_last_epoch = 7, 5e-5, 0
        for t in on:
            getattr(ts, f"set_lambda_{t}")(LAM[t], *(("ortho",) if t == "fft" else ()))
        return ts

    m = model()
    src = step(m, TERMS)
    entry = export_checkpoint(m, src, epoch=3)["m2t_loss"]
    assert list(entry) == ["pixel_loss", "param", "lambda_ssim", "lambda_msssim", "lambda_fft", "fft_norm", "lambda_vif", "lambda_perceptual",
                           "perceptual_criterion", "perceptual_weights", "perceptual_resize"]
    assert entry == {"pixel_loss": "l1", "param": None, "lambda_ssim": 0.1, "lambda_msssim": 0.16, "lambda_fft": 0.2, "fft_norm": "ortho",
                     "lambda_vif": 0.05, "lambda_perceptual": 0.03, "perceptual_criterion": "sl1",
                     "perceptual_weights": [1.0, 0.5, 0.0, 2.0, 1.5], "perceptual_resize": False}
    assert "m2t_loss" not in export_checkpoint(m, step(m, ()), epoch=3)       # every weight 0: no entry
    dst = step(model(), ())
    dst.perceptual_loss.weights, dst.perceptual_loss.criterion = [1.0] * 5, "l1"
    assert import_checkpoint(export_checkpoint(m, src, epoch=3), dst.model, dst) == 4
    assert [getattr(dst, f"lambda_{t}") for t in TERMS] == [LAM[t] for t in TERMS] and dst.fft_norm == "ortho"
    p = dst.perceptual_loss
    assert (p.criterion, p.weights, p.resize) == ("sl1", [1.0, 0.5, 0.0, 2.0, 1.5], False)
    assert export_checkpoint(m, dst, epoch=3)["m2t_loss"] == entry
    # a stand-in without the setters receives the attributes of the table's terms
    plain = types.SimpleNamespace(lr=1.0, step_count=0, exp_avg=torch.zeros_like(m.flat_params), exp_avg_sq=torch.zeros_like(m.flat_params),
                                  scheduler_last_epoch=0, set_lr=lambda lr: None)
    four = {k: v for k, v in export_checkpoint(m, step(m, TERMS[:4]), epoch=3).items()}
    import_checkpoint(four, model(), plain)
    assert [getattr(plain, f"lambda_{t}") for t in TERMS[:4]] == [LAM[t] for t in TERMS[:4]] and plain.fft_norm == "ortho"
