"""-m gpu: the optimizer options of TrainStep -- gradient-norm clipping, weight decay, EMA weights, the non-finite skip -- down to
m2t_grad_norm and m2t_adam_step_ex (m2trans_amd/csrc/k_optim.hip).

Yardsticks: numpy fp64 on the same fp32 data for the norm; for the step the fp64 evaluation and the fp32 restatement of the
kernel's rounding points in tests/optim_ref.py (checked against torch's own Adam by tests/test_optim_cpu.py), with the project's
"3x the CPU emulation of the kernel's rounding points" rule; torch.equal wherever two arms of this build must agree (no kernel
of the step uses atomics: a differing bit is a defect, not noise).  Every wait for the device has a time limit of its own; a
step that does not finish ends the whole session (nothing more is started on the device).  NaN in a gradient buffer is data."""
import io
import time

import numpy as np
import pytest
import torch

from oracle import m2trans_oracle as O
from tests import optim_ref as R
from tests.gpu_util import assert_flat_equal, build_model

pytestmark = pytest.mark.gpu

LR = 1e-3
B1, B2, EPS = 0.9, 0.999, 1e-8
ULP32 = 2.0 ** -23
OFF = {"max_grad_norm": None, "weight_decay": 0.0, "decoupled_weight_decay": False, "ema_decay": None, "skip_nonfinite": False,
       "track_grad_norm": False}
ALL_ON = {"max_grad_norm": 0.05, "weight_decay": 1e-2, "decoupled_weight_decay": True, "ema_decay": 0.9, "skip_nonfinite": True}


def _wait(seconds: float, what: str):
    """The time limit of one device step: poll an event recorded behind it; past the limit the session ends."""
    ev = torch.cuda.Event()
    ev.record()
    end = time.monotonic() + seconds
    while not ev.query():
        if time.monotonic() > end:
            pytest.exit(f"{what}: the device did not finish within {seconds} s; nothing more is started on it", returncode=3)
        time.sleep(0.002)


def _grad_norm(g, n, rec, ws, grad_scale=1.0, max_norm=0.0, skip=0, step=1):
    from m2trans_amd import _lib
    return _lib.load().m2t_grad_norm(_lib.ptr(g), n, grad_scale, max_norm, skip, step, B1, B2, _lib.ptr(rec), _lib.ptr(ws),
                                     _lib.stream_ptr())


def _workspace():
    from m2trans_amd import _lib
    return torch.empty(_lib.load().m2t_grad_norm_workspace_bytes() // 8, dtype=torch.float64, device="cuda")


def _batch(B, H, W, scale, step):
    return (O.closed_form_image(B, 3, H, W, phase=0.37 * step).cuda(),
            O.closed_form_image(B, 3, H * scale, W * scale, phase=0.7 + 0.91 * step).cuda())


def _twins(scale, nb, dtype):
    m_a, p = build_model(scale, nb, dtype)
    m_b, _ = build_model(scale, nb, dtype, params=p)
    assert torch.equal(m_a.flat_params, m_b.flat_params)
    return m_a, m_b


def _state(ts):
    """(p, m, v, ema, record) as detached copies."""
    c = lambda t: None if t is None else t.detach().clone()
    return c(ts.model.flat_params), c(ts.exp_avg), c(ts.exp_avg_sq), c(ts.ema_params), c(ts.optim_record)


def _assert_state_equal(tag, ts_a, ts_b, record=True):
    m = ts_a.model
    assert_flat_equal(m, m.flat_params, ts_b.model.flat_params, f"{tag}: parameters")
    assert_flat_equal(m, ts_a.exp_avg, ts_b.exp_avg, f"{tag}: exp_avg")
    assert_flat_equal(m, ts_a.exp_avg_sq, ts_b.exp_avg_sq, f"{tag}: exp_avg_sq")
    if ts_a.ema_params is not None or ts_b.ema_params is not None:
        assert_flat_equal(m, ts_a.ema_params, ts_b.ema_params, f"{tag}: ema")
    if record and (ts_a.optim_record is not None or ts_b.optim_record is not None):
        assert torch.equal(ts_a.optim_record, ts_b.optim_record), f"{tag}: record {ts_a.optim_record.tolist()} vs {ts_b.optim_record.tolist()}"


# ------------------------------------------------------------------------------------------------------------------ the norm
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 3629760])
def test_grad_norm_against_fp64_for_every_size_and_alignment(n):
    """sqrt(sum (grad_scale g)^2) against numpy fp64 on the same fp32 data, relative error <= 2 ulp of fp32 (the accumulation is
    fp64: only the final rounding is left), for pointers offset by 0..3 floats from a 16-byte boundary; two calls give the same
    bits; the gradient is not written; an inf or a NaN anywhere makes finite = 0 (and with skip_nonfinite, applied = 0)."""
    gen = torch.Generator(device="cuda").manual_seed(n + 11)
    PAD = 8
    ws = _workspace()
    for off in range(4):
        base = torch.randn(n + 2 * PAD, generator=gen, device="cuda") * torch.exp2(
            torch.randint(-12, 12, (n + 2 * PAD,), generator=gen, device="cuda").float())
        assert base.data_ptr() % 16 == 0
        g = base[4 + off:4 + off + n]
        assert g.data_ptr() % 16 == 4 * off
        before = base.clone()
        host = g.cpu().numpy()
        for gs in (1.0, 0.5):
            want = R.norm64(host, gs)
            recs = []
            for _ in range(2):
                rec = torch.zeros(8, dtype=torch.float64, device="cuda")
                ws.fill_(float("nan"))
                assert _grad_norm(g, n, rec, ws, grad_scale=gs, max_norm=1.0, step=3) == 0
                _wait(30, f"m2t_grad_norm n {n}")
                recs.append(rec.cpu())
            tag = f"n {n}, offset {off}, grad_scale {gs}"
            got = float(recs[0][0])
            print(f"{tag}: norm {got!r}, fp64 {want!r}, rel {abs(got - want) / want:.3e}")
            assert abs(got - want) <= 2 * ULP32 * want, tag
            assert torch.equal(recs[0], recs[1]), f"{tag}: two calls differ: {recs[0].tolist()} vs {recs[1].tolist()}"
            assert recs[0][1] == 1.0 and recs[0][3] == 1.0 and recs[0][4] == 0.0 and recs[0][7] == 3.0, (tag, recs[0].tolist())
            c64 = min(1.0, 1.0 / (want + 1e-6))
            assert abs(float(recs[0][2]) - c64) <= 2 * float(np.spacing(np.float32(c64))), (tag, float(recs[0][2]), c64)
            bc1, bc2s = R.bias_terms(B1, B2, 3)
            assert abs(float(recs[0][5]) - bc1) <= 1e-14 and abs(float(recs[0][6]) - bc2s) <= 1e-14, tag
        assert torch.equal(base, before), f"offset {off}: the gradient buffer was written"
        # non-finite data is data: the flag, and the skip decision with its running count
        for bad in (float("inf"), float("nan")):
            for pos in sorted({0, n // 2, n - 1}):
                g2 = base.clone()
                g2[4 + off + pos] = bad
                rec = torch.zeros(8, dtype=torch.float64, device="cuda")
                for call in (1, 2):
                    assert _grad_norm(g2[4 + off:4 + off + n], n, rec, ws, max_norm=1.0, skip=1, step=5) == 0
                    _wait(30, f"m2t_grad_norm n {n} with {bad}")
                    r = rec.cpu()
                    assert r[1] == 0.0 and r[3] == 0.0 and r[4] == float(call) and r[7] == 5.0 - call, (bad, pos, r.tolist())
                    assert not np.isfinite(float(r[0]))
                rec.zero_()
                assert _grad_norm(g2[4 + off:4 + off + n], n, rec, ws, max_norm=1.0, skip=0, step=5) == 0
                _wait(30, f"m2t_grad_norm n {n} with {bad}, no skip")
                r = rec.cpu()
                assert r[1] == 0.0 and r[3] == 1.0 and r[4] == 0.0, (bad, pos, r.tolist())


# ------------------------------------------------------------------------------------------------------------- step parity
PARITY_SETS = [("none", dict(track_grad_norm=True)),
               ("clip", dict(max_grad_norm=0.05)),
               ("clip_coupled", dict(max_grad_norm=0.05, weight_decay=1e-2)),
               ("clip_decoupled", dict(max_grad_norm=0.05, weight_decay=1e-2, decoupled_weight_decay=True)),
               ("clip_decoupled_ema", dict(max_grad_norm=0.05, weight_decay=1e-2, decoupled_weight_decay=True, ema_decay=0.9))]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name,opts", PARITY_SETS, ids=[s[0] for s in PARITY_SETS])
def test_step_parity_against_fp64_and_the_restatement(name, opts, dtype):
    """K = 4 teacher-forced optimizer steps on the real gradients of a 2-block model: every step's inputs (p, g, m, v, ema as the
    device holds them, the coefficient the record holds) go through tests/optim_ref.py's fp64 evaluation and fp32 restatement.
    Gates, computed here from those two: p within 2 ulp(p) + 3x the restatement's own worst excess over 2 ulp(p) on these
    inputs (elements where coupled decay cancels left out, their share capped at 1e-3); m, v, ema within 3x the restatement's
    worst deviation in their units (2^-24 of the sum of their terms' magnitudes).  The norm against fp64 and the coefficient
    against min(1, max_norm / (norm64 + 1e-6)) to 2 ulp of fp32; the gradient buffer bit-unchanged by the step.
    ("none" runs the new kernels with the coefficient at 1: track_grad_norm alone.)"""
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H, W, K = 4, 2, 2, 32, 32, 4
    model, _ = build_model(scale, nb, dtype)
    ts = TrainStep(model, lr=LR, world_size=1, **opts)
    assert ts._optim_ex and ts.optim_record is not None
    max_norm, wd = opts.get("max_grad_norm"), opts.get("weight_decay", 0.0)
    decoupled, d = opts.get("decoupled_weight_decay", False), opts.get("ema_decay")
    clipped = 0
    for step in range(1, K + 1):
        x, hr = _batch(B, H, W, scale, step)
        ts.forward_backward(x, hr)
        ts.all_reduce_grads()
        _wait(120, f"{name} {dtype} step {step}: forward + backward")
        np_ = lambda t: None if t is None else t.detach().cpu().numpy().copy()
        p0, g0, m0, v0, e0 = np_(model.flat_params), np_(ts.grads), np_(ts.exp_avg), np_(ts.exp_avg_sq), np_(ts.ema_params)
        assert np.isfinite(g0).all()
        ts.optimizer_step()
        _wait(60, f"{name} {dtype} step {step}: optimizer")
        got = (np_(model.flat_params), np_(ts.exp_avg), np_(ts.exp_avg_sq), np_(ts.ema_params))
        rec = ts.optim_record.cpu().numpy()
        tag = f"{name} {dtype} step {step}"
        assert np.array_equal(np_(ts.grads).view(np.uint32), g0.view(np.uint32)), f"{tag}: the step wrote the gradient buffer"
        # the record
        n64 = R.norm64(g0)
        assert abs(rec[0] - n64) <= 2 * ULP32 * n64, (tag, rec[0], n64)
        c64 = 1.0 if max_norm is None else min(1.0, max_norm / (n64 + 1e-6))
        coef = float(rec[2])
        assert abs(coef - c64) <= 2 * float(np.spacing(np.float32(c64))), (tag, coef, c64)
        assert float(ts.grad_norm) == rec[0] and float(ts.clip_coef) == coef and float(ts.skipped_steps) == 0.0
        assert rec[1] == 1.0 and rec[3] == 1.0 and rec[4] == 0.0 and rec[7] == float(step), (tag, rec.tolist())
        clipped += coef < 1.0
        # the step
        kw = dict(lr=LR, b1=B1, b2=B2, eps=EPS, t=step, coef=coef, wd=wd, decoupled=decoupled, ema_decay=d)
        r32, r64 = R.step_f32(p0, g0, m0, v0, e0, **kw), R.step_f64(p0, g0, m0, v0, e0, **kw)
        own, dev = R.deviations(r32, r64), R.deviations(got, r64)
        keep = ~R.cancelled(r64)
        left_out = 1.0 - keep.mean()
        same = {k: float(np.mean(a.view(np.uint32) == b.view(np.uint32))) for k, a, b in
                zip("pmve", got, r32) if a is not None}
        print(f"{tag}: norm {rec[0]:.6g} coef {coef:.6g}; bit-equal to the restatement {same}; cancelled share {left_out:.2e}")
        assert left_out <= R.CANCEL_CAP, (tag, left_out)
        own_p = float(own["p_beyond"][keep].max())
        excess = dev["p_abs"][keep] - 2.0 * R.ulp32(r64["p"])[keep]
        print(f"    p: restatement's worst excess over 2 ulp {own_p / LR:.3g} lr, kernel's {max(0.0, float(excess.max())) / LR:.3g} lr")
        assert float(excess.max()) <= 3.0 * own_p, (tag, float(excess.max()), own_p)
        for k in ("m", "v") + (("ema",) if d is not None else ()):
            print(f"    {k}: restatement {own[k].max():.3f}, kernel {dev[k].max():.3f} (units of 2^-24 of the terms' magnitudes)")
            assert dev[k].max() <= 3.0 * own[k].max(), (tag, k, float(dev[k].max()), float(own[k].max()))
    if max_norm is not None:
        assert clipped == K, f"{name}: max_grad_norm {max_norm} clipped {clipped} of {K} steps: the coefficient path was not exercised"


# ------------------------------------------------------------------------------------------------------------ default path
def test_every_option_at_its_default_is_the_plain_step():
    """TrainStep(model) and TrainStep(model, <every option spelled out at its default>): torch.equal weights, moments and loss
    over 3 steps, no EMA buffer, no record, and the one m2t_adam_step call."""
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H, W = 4, 2, 2, 32, 32
    m_a, m_b = _twins(scale, nb, "bf16")
    ts_a, ts_b = TrainStep(m_a, lr=LR, world_size=1), TrainStep(m_b, lr=LR, world_size=1, **OFF)
    for ts in (ts_a, ts_b):
        assert ts.ema_params is None and ts.optim_record is None and ts._norm_ws is None and not ts._optim_ex
        assert ts.grad_norm is None and ts.clip_coef is None and ts.skipped_steps is None
    for step in range(1, 4):
        x, hr = _batch(B, H, W, scale, step)
        la, lb = ts_a.step(x, hr).clone(), ts_b.step(x, hr).clone()
        _wait(120, f"default path step {step}")
        assert torch.equal(la, lb) and bool(torch.isfinite(la).all())
        _assert_state_equal(f"default path step {step}", ts_a, ts_b)
    assert ts_a.applied_step_count() == ts_b.applied_step_count() == 3


# -------------------------------------------------------------------------------------------------------------------- skip
def test_a_nonfinite_gradient_is_skipped_and_the_next_step_is_the_twins():
    """skip_nonfinite=True: a step whose gradient buffer carries one NaN leaves p, m, v and ema bit-identical and raises
    skipped_steps by 1; the next clean step equals, bit for bit, the step of a twin that never saw the NaN (the bias correction
    comes from the applied count).  skip_nonfinite=False: the NaN propagates, as in torch."""
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H, W = 4, 2, 2, 32, 32
    m_a, m_b = _twins(scale, nb, "bf16")
    ts_a, ts_b = TrainStep(m_a, lr=LR, world_size=1, **ALL_ON), TrainStep(m_b, lr=LR, world_size=1, **ALL_ON)
    x, hr = _batch(B, H, W, scale, 1)
    ts_a.step(x, hr), ts_b.step(x, hr)
    _wait(120, "skip: step 1")
    _assert_state_equal("skip: step 1", ts_a, ts_b)
    # arm A meets a NaN
    x, hr = _batch(B, H, W, scale, 2)
    ts_a.forward_backward(x, hr)
    ts_a.all_reduce_grads()
    ts_a.grads[ts_a.grads.numel() // 3] = float("nan")
    before = _state(ts_a)
    ts_a.optimizer_step()
    _wait(120, "skip: the step with the NaN")
    after = _state(ts_a)
    for what, a, b in zip(("parameters", "exp_avg", "exp_avg_sq", "ema"), before, after):
        assert_flat_equal(m_a, a, b, f"skipped step: {what}")
    assert float(ts_a.skipped_steps) == 1.0 and float(before[4][4]) == 0.0
    rec = ts_a.optim_record.cpu()
    assert rec[1] == 0.0 and rec[3] == 0.0 and not np.isfinite(float(rec[0])), rec.tolist()
    assert ts_a.step_count == 2 and ts_a.applied_step_count() == 1 and ts_b.applied_step_count() == 1
    # the next clean step of both
    x, hr = _batch(B, H, W, scale, 3)
    la, lb = ts_a.step(x, hr).clone(), ts_b.step(x, hr).clone()
    _wait(120, "skip: the clean step after")
    assert torch.equal(la, lb)
    _assert_state_equal("clean step after the skip", ts_a, ts_b, record=False)
    ra, rb = ts_a.optim_record.cpu(), ts_b.optim_record.cpu()
    assert torch.equal(ra[[0, 1, 2, 3, 5, 6, 7]], rb[[0, 1, 2, 3, 5, 6, 7]]) and ra[4] == 1.0 and rb[4] == 0.0 and ra[7] == 2.0
    assert (ts_a.step_count, ts_a.applied_step_count(), ts_b.step_count) == (3, 2, 2)
    # without the skip the NaN propagates
    m_c, _ = build_model(scale, nb, "bf16")
    ts_c = TrainStep(m_c, lr=LR, world_size=1, **dict(ALL_ON, skip_nonfinite=False))
    ts_c.forward_backward(x, hr)
    idx = ts_c.grads.numel() // 3
    ts_c.grads[idx] = float("nan")
    ts_c.optimizer_step()
    _wait(120, "skip off: the step with the NaN")
    assert bool(torch.isnan(m_c.flat_params[idx])) and bool(torch.isnan(ts_c.exp_avg[idx])) and bool(torch.isnan(ts_c.ema_params[idx]))
    rec = ts_c.optim_record.cpu()
    assert rec[1] == 0.0 and rec[3] == 1.0 and rec[4] == 0.0, rec.tolist()


# ------------------------------------------------------------------------------------------------------------- composition
def _chunk_grads(model, cx, chr_, divisor):
    """(loss [1], gradients) of one chunk through m2t_forward, m2t_l1_loss_deferred, m2t_backward into a fresh buffer."""
    from m2trans_amd import _lib
    lib = _lib.load()
    cx, chr_ = cx.contiguous().float(), chr_.contiguous().float()
    plan = model._plan_for(cx)
    plan.gen += 1
    plan.trained = True
    g = torch.full_like(model.flat_params, float("nan"))
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=cx.device)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(cx), None, float(model.rgb_range), 1, ws, st), "m2t_forward")
    _lib.check(lib.m2t_l1_loss_deferred(plan.handle, _lib.ptr(chr_), 1.0, divisor, float(model.rgb_range), _lib.ptr(loss), ws, st),
               "m2t_l1_loss_deferred")
    _lib.check(lib.m2t_backward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(cx), _lib.ptr(g), ws, st), "m2t_backward")
    return loss, g


def test_accumulation_with_clipping_equals_the_by_hand_arm():
    """accum_steps = 2 with clipping + coupled decay + EMA against the by-hand arm: the chunk gradients summed by torch, then
    m2t_grad_norm + m2t_adam_step_ex on the sum.  torch.equal over 3 optimizer steps: the norm is that of the ACCUMULATED buffer."""
    from m2trans_amd import _lib
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H, W, k = 4, 2, 4, 32, 32, 2
    opts = dict(max_grad_norm=0.05, weight_decay=1e-2, ema_decay=0.9)
    m_a, m_b = _twins(scale, nb, "bf16")
    ts = TrainStep(m_a, lr=LR, world_size=1, accum_steps=k, **opts)
    lib = _lib.load()
    hm, hv, hema = torch.zeros_like(m_b.flat_params), torch.zeros_like(m_b.flat_params), m_b.flat_params.detach().clone()
    hrec, hws = torch.zeros(8, dtype=torch.float64, device="cuda"), _workspace()
    n = m_b.flat_params.numel()
    for step in range(1, 4):
        x, hr = _batch(B, H, W, scale, step)
        la = ts.step(x, hr).clone()
        b = B // k
        (l0, g0), (l1, g1) = (_chunk_grads(m_b, x[i * b:(i + 1) * b], hr[i * b:(i + 1) * b], float(hr.numel())) for i in range(k))
        lb, gsum = l0 + l1, g0 + g1
        _lib.check(lib.m2t_grad_norm(_lib.ptr(gsum), n, 1.0, opts["max_grad_norm"], 0, step, B1, B2, _lib.ptr(hrec), _lib.ptr(hws),
                                     _lib.stream_ptr()), "m2t_grad_norm")
        _lib.check(lib.m2t_adam_step_ex(_lib.ptr(m_b.flat_params), _lib.ptr(gsum), _lib.ptr(hm), _lib.ptr(hv), n, LR, B1, B2, EPS, step,
                                        1.0, _lib.ptr(hema), opts["weight_decay"], 0, opts["ema_decay"], _lib.ptr(hrec),
                                        _lib.stream_ptr()), "m2t_adam_step_ex")
        _wait(120, f"accumulation + clipping step {step}")
        tag = f"accum + clip step {step}"
        assert torch.equal(la, lb) and float(ts.clip_coef) < 1.0, (tag, float(ts.clip_coef))
        assert_flat_equal(m_a, ts.grads, gsum, f"{tag}: gradients")
        assert_flat_equal(m_a, m_a.flat_params, m_b.flat_params, f"{tag}: parameters")
        assert_flat_equal(m_a, ts.exp_avg, hm, f"{tag}: exp_avg")
        assert_flat_equal(m_a, ts.exp_avg_sq, hv, f"{tag}: exp_avg_sq")
        assert_flat_equal(m_a, ts.ema_params, hema, f"{tag}: ema")
        assert torch.equal(ts.optim_record, hrec), tag
    # swap_ema in the middle of a cycle raises
    ts.forward_backward(x[:b], hr[:b])
    with pytest.raises(_lib.M2TError, match="accumulation cycle"):
        ts.swap_ema()
    ts.forward_backward(x[b:], hr[b:])
    ts.optimizer_step()
    _wait(120, "accumulation: closing the cycle")


def test_communication_path_with_one_rank_equals_the_plain_path():
    """force_comm_path=True with one rank (the collectives are identities; the norm runs behind the compute stream's wait for
    the communication stream): bit for bit the plain path, every option on, 3 steps."""
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H, W = 4, 2, 2, 64, 64
    m_a, m_b = _twins(scale, nb, "bf16")
    ts_a = TrainStep(m_a, lr=LR, world_size=1, force_comm_path=True, **ALL_ON)
    ts_b = TrainStep(m_b, lr=LR, world_size=1, **ALL_ON)
    assert ts_a.overlap_comm and ts_b.bucket is None
    for step in range(1, 4):
        x, hr = _batch(B, H, W, scale, step)
        la, lb = ts_a.step(x, hr).clone(), ts_b.step(x, hr).clone()
        _wait(120, f"communication path step {step}")
        assert torch.equal(la, lb)
        _assert_state_equal(f"communication path step {step}", ts_a, ts_b)


# --------------------------------------------------------------------------------------------------------------------- EMA
def test_ema_swap_state_dict_and_zero_decay():
    from m2trans_amd import _lib
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H, W = 4, 2, 2, 32, 32
    model, _ = build_model(scale, nb, "bf16")
    ts = TrainStep(model, lr=LR, world_size=1, ema_decay=0.9)
    assert ts.optim_record is None and ts._optim_ex                  # EMA alone pays for no norm pass
    assert torch.equal(ts.ema_params, model.flat_params) and ts.ema_params.data_ptr() != model.flat_params.data_ptr()
    for step in range(1, 3):
        ts.step(*_batch(B, H, W, scale, step))
    _wait(120, "ema: two steps")
    p, e = model.flat_params.detach().clone(), ts.ema_params.clone()
    assert not torch.equal(p, e) and bool(torch.isfinite(e).all())
    ts.swap_ema()
    assert torch.equal(model.flat_params, e) and torch.equal(ts.ema_params, p)
    with torch.no_grad():
        sr_ema = model(_batch(B, H, W, scale, 9)[0])                 # the model runs on the EMA weights
    assert bool(torch.isfinite(sr_ema).all())
    ts.swap_ema()
    assert torch.equal(model.flat_params, p) and torch.equal(ts.ema_params, e)
    # the state dict: the model's own names, loadable strictly into a fresh model
    sd = ts.ema_state_dict()
    assert list(sd) == list(model.state_dict()) and len(sd) == 11 + 14 * nb
    fresh, _ = build_model(scale, nb, "bf16")
    fresh.load_state_dict(sd, strict=True)
    assert torch.equal(fresh.flat_params, e)
    for k in set(sd) - set(model._names):                            # the frozen MeanShift entries are the model's
        assert torch.equal(sd[k], model.state_dict()[k])
    # ema_decay = 0: the EMA equals the weights after every step
    m0, _ = build_model(scale, nb, "bf16")
    t0 = TrainStep(m0, lr=LR, world_size=1, ema_decay=0.0)
    for step in range(1, 4):
        t0.step(*_batch(B, H, W, scale, step))
        _wait(120, f"ema_decay 0 step {step}")
        assert torch.equal(t0.ema_params, m0.flat_params), f"ema_decay = 0, step {step}"
    with pytest.raises(_lib.M2TError, match="ema_decay=None"):
        TrainStep(build_model(scale, 1, "bf16")[0], lr=LR, world_size=1).ema_state_dict()


# -------------------------------------------------------------------------------------------------------------- checkpoint
def test_checkpoint_resume_with_every_option_on_is_bit_identical():
    """2 steps -> export_checkpoint -> torch.save / torch.load -> a FRESH model and a TrainStep built with every option at its
    default -> import_checkpoint -> 2 more steps == 4 uninterrupted steps, bit for bit: weights, moments, EMA and record."""
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H, W = 4, 2, 2, 32, 32
    m_a, m_b = _twins(scale, nb, "bf16")
    ts_a, ts_b = TrainStep(m_a, lr=LR, world_size=1, **ALL_ON), TrainStep(m_b, lr=LR, world_size=1, **ALL_ON)
    for step in range(1, 3):
        x, hr = _batch(B, H, W, scale, step)
        ts_a.step(x, hr), ts_b.step(x, hr)
    _wait(120, "checkpoint: two steps")
    buf = io.BytesIO()
    torch.save(export_checkpoint(m_b, ts_b, epoch=1), buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    assert ck["m2t_optim"] == {"max_grad_norm": 0.05, "ema_decay": 0.9, "skip_nonfinite": True, "skipped_steps": 0}
    assert ck["optimizer_state_dict"]["param_groups"][0]["weight_decay"] == 1e-2
    m_c, _ = build_model(scale, nb, "bf16")
    m_c.flat_params.data.mul_(0.5)                                    # (not the weights of the checkpoint)
    ts_c = TrainStep(m_c, lr=5e-4, world_size=1)
    assert ts_c.ema_params is None and ts_c.optim_record is None
    import_checkpoint(ck, m_c, ts_c)
    assert (ts_c.max_grad_norm, ts_c.weight_decay, ts_c.decoupled_weight_decay, ts_c.ema_decay, ts_c.skip_nonfinite) == \
           (0.05, 1e-2, True, 0.9, True)
    assert ts_c.step_count == 2 and ts_c.lr == LR and float(ts_c.skipped_steps) == 0.0
    assert_flat_equal(m_a, m_c.flat_params, m_a.flat_params, "resume: loaded parameters")
    assert_flat_equal(m_a, ts_c.ema_params, ts_a.ema_params, "resume: loaded ema")
    for step in range(3, 5):
        x, hr = _batch(B, H, W, scale, step)
        la, lc = ts_a.step(x, hr).clone(), ts_c.step(x, hr).clone()
        _wait(120, f"checkpoint: step {step}")
        assert torch.equal(la, lc)
        _assert_state_equal(f"resume step {step}", ts_a, ts_c)
    assert float(ts_c.optim_record[7]) == 4.0 and float(ts_c.clip_coef) < 1.0
