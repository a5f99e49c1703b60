"""-m gpu: gradient accumulation in the fused step driver, TrainStep(accum_steps=k).

One optimizer step consumes k equal micro-batches; calls 2..k of a cycle hand m2t_backward a second flat buffer and the deferred
L1 loss a second slot, and ONE m2t_grad_accumulate per micro-batch adds both to the first call's.  Every addition is an ordered
fp32 addition and no kernel of the step uses atomics, so every comparison between two arms of this build is torch.equal: a
differing bit is a defect, not noise.  The yardsticks are torch's ``acc += g`` (the op), the entry points that exist without the
feature driven by hand (the composition: forward, deferred L1 with the whole batch's divisor, backward into a fresh buffer, the
sum taken by torch, m2t_adam_step on the sum) and the CPU oracle on the FULL batch (fp32, tolerances of tests/test_gpu_model.py)."""
import ctypes as C

import pytest
import torch

from oracle import m2trans_oracle as O
from oracle import swin_oracle as S
from tests.gpu_util import assert_flat_equal, build_model, poison_float_regions, rel, set_options

pytestmark = pytest.mark.gpu

K_OPT = 3            # optimizer steps per comparison: step 1 runs the first-backward schedule of the plan, 2.. the steady state
LR = 1e-3


def _image(B, h, w, phase):
    """B different closed-form images; beyond four samples shifted copies of the first four, made on the device (as
    tests/test_gpu_schedule.py does: the CPU generator would dominate the run)."""
    base = O.closed_form_image(min(B, 4), 3, h, w, phase=phase).cuda()
    if B <= 4:
        return base
    return torch.cat([torch.roll(base, shifts=(3 * g, 5 * g), dims=(2, 3)) for g in range((B + 3) // 4)])[:B].contiguous()


def _batch(B, H, W, scale, step):
    return _image(B, H, W, 0.37 * step), _image(B, H * scale, W * scale, 0.7 + 0.91 * step)


def _twins(scale, nb, dtype):
    m_a, p = build_model(scale, nb, dtype)
    m_b, _ = build_model(scale, nb, dtype, params=p)
    assert torch.equal(m_a.flat_params, m_b.flat_params)
    return m_a, m_b, p


class _ByHand:
    """Arm B: the step of a batch cut into k chunks through the entry points that exist without the feature."""

    def __init__(self, model, lr=LR):
        self.model, self.lr, self.step_count = model, lr, 0
        self.exp_avg = torch.zeros_like(model.flat_params)
        self.exp_avg_sq = torch.zeros_like(model.flat_params)
        self.grads = None
        self.chunk_grads = []

    def chunk(self, cx, chr_, divisor):
        """(loss [1], gradients) of one chunk: m2t_forward, m2t_l1_loss_deferred, m2t_backward into a fresh buffer."""
        from m2trans_amd import _lib
        lib, m = _lib.load(), self.model
        cx, chr_ = cx.contiguous().float(), chr_.contiguous().float()
        plan = m._plan_for(cx)
        plan.gen += 1
        plan.trained = True
        g = torch.full_like(m.flat_params, float("nan"))
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device=cx.device)
        ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
        _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(m.flat_params), _lib.ptr(cx), None, float(m.rgb_range), 1, ws, st), "m2t_forward")
        _lib.check(lib.m2t_l1_loss_deferred(plan.handle, _lib.ptr(chr_), 1.0, divisor, float(m.rgb_range), _lib.ptr(loss), ws, st),
                   "m2t_l1_loss_deferred")
        _lib.check(lib.m2t_backward(plan.handle, _lib.ptr(m.flat_params), _lib.ptr(cx), _lib.ptr(g), ws, st), "m2t_backward")
        return loss, g

    def step(self, x, hr, k):
        from m2trans_amd import _lib
        B = x.shape[0]
        b = B // k
        assert b * k == B
        divisor = float(hr.numel())                               # the whole batch's element count
        loss, gsum, self.chunk_grads = None, None, []
        for i in range(k):
            li, gi = self.chunk(x[i * b:(i + 1) * b], hr[i * b:(i + 1) * b], divisor)
            self.chunk_grads.append(gi)
            loss = li if loss is None else loss + li              # ((l_0 + l_1) + l_2) + ... in fp32, by torch
            gsum = gi if gsum is None else gsum + gi
        self.grads = gsum
        self.step_count += 1
        m = self.model
        _lib.check(_lib.load().m2t_adam_step(_lib.ptr(m.flat_params), _lib.ptr(gsum), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                                             gsum.numel(), self.lr, 0.9, 0.999, 1e-8, self.step_count, 1.0, _lib.stream_ptr()),
                   "m2t_adam_step")
        return loss


def _compare(tag, ts, ref, loss_a, loss_b):
    """ts: a TrainStep; ref: a TrainStep or a _ByHand.  Loss, gradients, parameters and both moments, torch.equal."""
    torch.cuda.synchronize()
    model = ts.model
    assert bool(torch.isfinite(loss_a).all()) and bool(torch.isfinite(ts.grads).all()), f"{tag}: non-finite loss or gradient"
    assert torch.equal(loss_a, loss_b), f"{tag}: loss {float(loss_a)!r} vs {float(loss_b)!r}"
    assert_flat_equal(model, ts.grads, ref.grads, f"{tag}: gradients")
    assert_flat_equal(model, model.flat_params, ref.model.flat_params, f"{tag}: parameters")
    assert_flat_equal(model, ts.exp_avg, ref.exp_avg, f"{tag}: exp_avg")
    assert_flat_equal(model, ts.exp_avg_sq, ref.exp_avg_sq, f"{tag}: exp_avg_sq")


# ------------------------------------------------------------------ 3. the op alone
def _accumulate(acc, g, n, loss_acc=None, loss_part=None):
    from m2trans_amd import _lib
    return _lib.load().m2t_grad_accumulate(_lib.ptr(acc), _lib.ptr(g), n, _lib.ptr(loss_acc), _lib.ptr(loss_part), _lib.stream_ptr())


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 3629760])
def test_grad_accumulate_is_torchs_inplace_add_for_every_size_and_alignment(n):
    """acc += g against torch, torch.equal, for both pointers offset by 0..3 floats from a 16-byte boundary (equal offsets: the
    16-byte path with its scalar head and tail; unequal ones: the scalar loop), with and without the loss pair; the elements on
    either side of the range keep their values."""
    gen = torch.Generator(device="cuda").manual_seed(n + 1)
    PAD = 8
    for oa in range(4):
        for og in range(4):
            for with_loss in (False, True):
                # (magnitudes over many binades: the sum is rounded in nearly every element)
                base = torch.randn(n + 2 * PAD, generator=gen, device="cuda") * torch.exp2(torch.randint(-12, 12, (n + 2 * PAD,), generator=gen, device="cuda").float())
                gbase = torch.randn(n + 2 * PAD, generator=gen, device="cuda") * torch.exp2(torch.randint(-12, 12, (n + 2 * PAD,), generator=gen, device="cuda").float())
                assert base.data_ptr() % 16 == 0 and gbase.data_ptr() % 16 == 0
                lo_a, lo_g = 4 + oa, 4 + og
                acc, g = base[lo_a:lo_a + n], gbase[lo_g:lo_g + n]
                if n:
                    assert acc.data_ptr() % 16 == 4 * oa and g.data_ptr() % 16 == 4 * og
                want = base.clone()
                want[lo_a:lo_a + n] += g
                gwant = gbase.clone()
                la = torch.tensor([0.8125 + n], device="cuda") if with_loss else None
                lp = torch.tensor([1.0 / 3.0], device="cuda") if with_loss else None
                lwant = (la + lp) if with_loss else None
                rc = _accumulate(acc, g, n, la, lp)
                torch.cuda.synchronize()
                tag = f"n {n}, acc offset {oa}, g offset {og}, loss pair {with_loss}"
                assert rc == 0, tag
                assert torch.equal(base, want), f"{tag}: {int((base != want).sum())} elements differ (range or its surroundings)"
                assert torch.equal(gbase, gwant), f"{tag}: g was written"
                if with_loss:
                    assert torch.equal(la, lwant), tag
                    assert float(lp) == float(torch.tensor(1.0 / 3.0)), tag


def test_grad_accumulate_argument_errors():
    from m2trans_amd import _lib
    a = torch.ones(8, device="cuda")
    g = torch.ones(8, device="cuda")
    l0, l1 = torch.ones(1, device="cuda"), torch.ones(1, device="cuda")
    for args in ((None, g, 8, None, None), (a, None, 8, None, None), (a, g, -1, None, None), (a, g, 8, l0, None), (a, g, 8, None, l1)):
        rc = _accumulate(*args)
        assert rc != 0
        with pytest.raises(_lib.M2TError, match="m2t_grad_accumulate"):
            _lib.check(rc, "m2t_grad_accumulate")
    torch.cuda.synchronize()
    assert float(a.sum()) == 8 and float(l0) == 1 and float(l1) == 1            # nothing was enqueued
    assert _accumulate(None, None, 0) == 0                                      # n = 0: null pointers are legal
    assert _accumulate(None, None, 0, l0, l1) == 0                              # ... and the loss pair alone is added
    torch.cuda.synchronize()
    assert float(l0) == 2


# ------------------------------------------------------------------ 4. composition, bit for bit
COMPOSITION_CASES = [
    # dtype, scale, n_blocks, batch, k, H, W
    pytest.param("bf16", 4, 8, 32, 2, 128, 128, id="bf16-x4-2x16-bench-geometry"),
    pytest.param("bf16", 4, 8, 64, 2, 128, 128, id="bf16-x4-2x32-big-wgrad-tiles"),
    pytest.param("fp32", 4, 2, 8, 4, 32, 32, id="fp32-x4-4x2"),
    pytest.param("bf16", 3, 2, 4, 2, 64, 64, id="bf16-x3-2x2"),
    pytest.param("bf16", 2, 4, 4, 4, 40, 56, id="bf16-x2-4x1-reflect-padded"),
]


@pytest.mark.parametrize("dtype,scale,nb,B,k,H,W", COMPOSITION_CASES)
def test_accumulated_step_equals_the_existing_entry_points_summed_by_torch(dtype, scale, nb, B, k, H, W):
    from m2trans_amd.train_step import TrainStep
    m_a, m_b, _ = _twins(scale, nb, dtype)
    ts = TrainStep(m_a, lr=LR, world_size=1, accum_steps=k)
    ref = _ByHand(m_b)
    first = None
    for step in range(K_OPT):
        x, hr = _batch(B, H, W, scale, step)
        loss_a = ts.step(x, hr).clone()
        loss_b = ref.step(x, hr, k)
        _compare(f"optimizer step {step + 1} (TrainStep(accum_steps={k}) vs the entry points by hand)", ts, ref, loss_a, loss_b)
        assert ts.step_count == step + 1 and ts.micro_count == 0
        assert first is None or not torch.equal(loss_a, first), "the batches must differ from step to step"
        first = loss_a if first is None else first
    assert float(ts.grads.abs().max()) > 0
    assert len(m_a._plans) == 1, "every micro-batch runs through the one plan of the micro-batch shape"


# ------------------------------------------------------------------ 5. against the oracle on the FULL batch
@pytest.mark.parametrize("scale,nb,B,k,H0,W0", [(4, 2, 4, 2, 32, 32), (3, 1, 4, 4, 40, 56), (2, 1, 4, 2, 32, 32)])
def test_accumulated_cycle_vs_oracle_full_batch_fp32(scale, nb, B, k, H0, W0):
    """Every parameter gradient of one accumulated cycle <= 1e-4 (of the tensor's largest element) of the oracle's full-batch
    gradient, loss within 1e-5 (test_backward_fp32_every_parameter's gates); then two optimizer steps against O.adam_update on
    full-batch oracle gradients by the criterion of test_train_two_steps_vs_reference_golden: the UPDATE, 5 % of the two-step
    update size, on that test's tensors (first conv, a body bias, last conv -- Adam moves a weight whose true gradient is zero,
    such as a bias in front of an InstanceNorm, by +-lr on rounding noise, so not every tensor can be asked)."""
    from m2trans_amd.train_step import TrainStep
    lr = 1e-4
    model, p0 = build_model(scale, nb, "fp32")
    ts = TrainStep(model, lr=lr, world_size=1, accum_steps=k)
    p = {n: v.clone() for n, v in p0.items()}
    names = O.trainable_names(p)
    mo = {n: torch.zeros_like(p[n]) for n in names}
    vo = {n: torch.zeros_like(p[n]) for n in names}
    offs = model.param_offsets()
    for step in range(1, 3):
        x = O.closed_form_image(B, 3, H0, W0, phase=0.1 * step)
        hr = O.closed_form_image(B, 3, H0 * scale, W0 * scale, phase=0.7 + 0.1 * step)
        loss_o, _, g_o = O.l1_loss_and_grads(x, hr, p, scale, nb)
        loss = ts.step(x.cuda(), hr.cuda())
        torch.cuda.synchronize()
        print(f"step {step}: loss {float(loss):.7f} oracle {float(loss_o):.7f}")
        assert abs(float(loss) - float(loss_o)) < 1e-5
        if step == 1:
            rows = [(n, rel(ts.grads[o:o + cnt], g_o[n].reshape(-1))) for n, (o, cnt) in offs.items()]
            print(f"worst gradient tensor: {max(e for _, e in rows):.3e}")
            bad = [(n, e) for n, e in rows if not (e < 1e-4)]
            assert not bad, "\n".join(f"{n:40s} {e:.3e}" for n, e in bad)
        for n in names:
            p[n], mo[n], vo[n] = O.adam_update(p[n], g_o[n], mo[n], vo[n], step, lr)
    sd = model.state_dict()
    for name in ("head.weight", "body.0.feed_forward.0.bias", "tail.6.weight" if scale == 4 else "tail.3.weight"):
        d = float((sd[name].cpu() - p[name]).abs().max())
        print(f"{name}: update differs by {d:.3e} (two-step update size {2 * lr:.1e})")
        assert d < 0.05 * 2 * lr, name


# ------------------------------------------------------------------ 6. accum_steps = 1 is the step as it was
def test_accum_steps_one_is_the_plain_step():
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, H, W = 4, 4, 4, 64, 64
    m_a, m_b, _ = _twins(scale, nb, "bf16")
    ts_a = TrainStep(m_a, lr=LR, world_size=1, accum_steps=1)
    ts_b = TrainStep(m_b, lr=LR, world_size=1)
    for ts in (ts_a, ts_b):
        assert ts.accum_steps == 1 and ts.micro_grads is None and ts.micro_loss is None
    for step in range(2):
        x, hr = _batch(B, H, W, scale, step)
        la, lb = ts_a.step(x, hr).clone(), ts_b.step(x, hr).clone()
        _compare(f"step {step + 1} (accum_steps=1 vs default)", ts_a, ts_b, la, lb)
        assert ts_a.micro_count == 0
    # no cycle rule: forward_backward any number of times without an optimizer step, each call overwriting the last
    x7, hr7 = _batch(B, H, W, scale, 7)
    ts_a.forward_backward(*_batch(B, H, W, scale, 5))
    ts_a.forward_backward(*_batch(B, H, W, scale, 6))
    la = ts_a.forward_backward(x7, hr7).clone()
    lb = ts_b.forward_backward(x7, hr7).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    assert_flat_equal(m_a, ts_a.grads, ts_b.grads, "third forward_backward without an optimizer step")
    ts_a.all_reduce_grads()
    ts_a.optimizer_step()
    for bad in (0, -1, 1.5):
        with pytest.raises(Exception):
            TrainStep(m_a, accum_steps=bad)


# ------------------------------------------------------------------ 7. schedule and stale reads
def test_accumulated_cycle_two_stream_equals_one_stream():
    """k = 2 at the benchmark geometry per micro-batch (bf16 x4, 8 blocks, 2 x 16, 128 x 128): side_stream 1 against 0, bit for
    bit over K_OPT optimizer steps.  The accumulate kernel reads the micro buffer behind a backward whose last reductions run on
    the side stream, and the next micro-batch's side-stream launches write it again."""
    from m2trans_amd.train_step import TrainStep
    scale, nb, b, k, H, W = 4, 8, 16, 2, 128, 128
    m_a, m_b, _ = _twins(scale, nb, "bf16")
    shape = torch.empty(b, 3, H, W, device="cuda")
    plan_a = set_options(m_a, shape)
    plan_b = set_options(m_b, shape, side_stream=0)
    assert plan_a.query("opt:side_stream") == 1 and plan_b.query("opt:side_stream") == 0
    ts_a = TrainStep(m_a, lr=LR, world_size=1, accum_steps=k)
    ts_b = TrainStep(m_b, lr=LR, world_size=1, accum_steps=k)
    for step in range(K_OPT):
        x, hr = _batch(b * k, H, W, scale, step)
        la, lb = ts_a.step(x, hr).clone(), ts_b.step(x, hr).clone()
        _compare(f"optimizer step {step + 1} (two-stream vs one-stream, accum_steps={k})", ts_a, ts_b, la, lb)
    assert m_a._plan_for(shape) is plan_a and m_b._plan_for(shape) is plan_b


def test_accumulated_cycle_reads_nothing_stale():
    """Arm A drives the cycle through forward_backward with, before every micro-batch but the very first of the plan, 0xFF (NaN)
    in every floating-point workspace region, and before every micro-batch 0xFF in the micro buffer and the micro loss slot;
    arm B is step() on an untouched twin.  No bit of loss, gradients, parameters or moments may change."""
    from m2trans_amd.train_step import TrainStep
    scale, nb, b, k, H, W = 4, 8, 16, 2, 128, 128
    m_a, m_b, _ = _twins(scale, nb, "bf16")
    ts_a = TrainStep(m_a, lr=LR, world_size=1, accum_steps=k)
    ts_b = TrainStep(m_b, lr=LR, world_size=1, accum_steps=k)
    plan = m_a._plan_for(torch.empty(b, 3, H, W, device="cuda"))
    used = False
    for step in range(K_OPT):
        x, hr = _batch(b * k, H, W, scale, step)
        for i in range(k):
            torch.cuda.synchronize()
            if used:
                poison_float_regions(plan)
            ts_a.micro_grads.view(torch.uint8).fill_(0xFF)
            ts_a.micro_loss.view(torch.uint8).fill_(0xFF)
            la = ts_a.forward_backward(x[i * b:(i + 1) * b], hr[i * b:(i + 1) * b])
            used = True
        la = la.clone()
        ts_a.all_reduce_grads()
        ts_a.optimizer_step()
        lb = ts_b.step(x, hr).clone()
        _compare(f"optimizer step {step + 1} (poisoned between micro-batches vs untouched)", ts_a, ts_b, la, lb)


# ------------------------------------------------------------------ 8. the communication path, one rank
def test_accumulated_cycle_exchanges_once_per_optimizer_step():
    """Arm A: force_comm_path (bucket, communication stream, Adam behind it) with one rank, default options; arm B: side_stream = 0
    and no bucket -- the set-up of test_communication_stream_live_equals_one_stream_step, at k = 2.  Bit for bit over K_OPT
    optimizer steps, and per optimizer step the ranges handed to the collective cover the gradient buffer exactly once (not once
    per micro-batch)."""
    from m2trans_amd.train_step import TrainStep
    scale, nb, b, k, H, W = 4, 8, 16, 2, 128, 128
    m_a, m_b, _ = _twins(scale, nb, "bf16")
    set_options(m_b, torch.empty(b, 3, H, W, device="cuda"), side_stream=0)
    ts_a = TrainStep(m_a, lr=LR, world_size=1, force_comm_path=True, accum_steps=k)
    ts_b = TrainStep(m_b, lr=LR, world_size=1, accum_steps=k)
    assert ts_a.overlap_comm and ts_a.comm_stream is not None and ts_b.bucket is None
    calls = []
    whole, ranged = ts_a.bucket.all_reduce, ts_a.bucket.all_reduce_range
    ts_a.bucket.all_reduce = lambda *a, **kw: (calls.append((0, ts_a.grads.numel())), whole(*a, **kw))[1]
    ts_a.bucket.all_reduce_range = lambda lo, hi: (calls.append((lo, hi)), ranged(lo, hi))[1]
    for step in range(K_OPT):
        x, hr = _batch(b * k, H, W, scale, step)
        del calls[:]
        la, lb = ts_a.step(x, hr).clone(), ts_b.step(x, hr).clone()
        _compare(f"optimizer step {step + 1} (communication path vs none, accum_steps={k})", ts_a, ts_b, la, lb)
        covered = sorted(c for c in calls if c[1] > c[0])
        assert covered and covered[0][0] == 0 and covered[-1][1] == ts_a.grads.numel(), covered
        assert all(covered[i][1] == covered[i + 1][0] for i in range(len(covered) - 1)), f"exchanged more or less than once: {covered}"


# ------------------------------------------------------------------ 9. SemanticLoss
def _semantic(differentiable, max_batch, caps):
    from m2trans_amd.losses import SemanticLoss
    g = torch.Generator().manual_seed(8)
    table = {c: torch.randn(512, generator=g) for c in caps}
    sl = SemanticLoss(criterion="l1", N_patches=3, device="cuda", compute_dtype="bf16", max_batch=max_batch, differentiable=differentiable)
    sl.load_image_encoder(S.closed_form_swin_params())
    sl.set_text_features(table)
    return sl


def test_semantic_constant_term_adds_up_over_the_cycle():
    """Batch 4 = 2 x 2, closed-form Swin-T weights: with the same torch.manual_seed the per-sample values of the chunked cycle
    equal, bit for bit, those of ONE semantic_loss.batch call over the four samples (on the SR images of the same two forward
    passes): the crop origins are drawn in sample order, nothing couples samples.  clip_loss is their sum times lambda_clip (two
    fp32 partial sums against one sum of four positive values: 1e-6 relative), loss = l1_loss + clip_loss."""
    from m2trans_amd.train_step import TrainStep
    scale, nb, B, k, H, W = 4, 4, 4, 2, 128, 128
    b, lam = B // k, 0.01
    caps = [f"c{i}" for i in range(B)]
    m_a, m_b, _ = _twins(scale, nb, "bf16")
    sl_a, sl_b = _semantic(False, b, caps), _semantic(False, B, caps)          # (max_batch applies to the chunk)
    ts = TrainStep(m_a, lr=LR, world_size=1, semantic_loss=sl_a, lambda_clip=lam, accum_steps=k)
    x, hr = _batch(B, H, W, scale, 1)
    torch.manual_seed(1234)
    per = []
    for i in range(k):
        loss = ts.forward_backward(x[i * b:(i + 1) * b], hr[i * b:(i + 1) * b], caps[i * b:(i + 1) * b])
        torch.cuda.synchronize()
        per.append(sl_a.last_per_sample.clone())
    per = torch.cat(per)
    from m2trans_amd import _lib
    sr = torch.empty_like(hr)
    for i in range(k):                                     # the forward call of the step, on the twin: sr of each chunk
        cx = x[i * b:(i + 1) * b].contiguous()
        plan = m_b._plan_for(cx)
        plan.gen += 1
        _lib.check(_lib.load().m2t_forward(plan.handle, _lib.ptr(m_b.flat_params), _lib.ptr(cx), _lib.ptr(sr[i * b:(i + 1) * b]), 1.0, 1,
                                           _lib.ptr(plan.workspace), _lib.stream_ptr()), "m2t_forward")
    torch.manual_seed(1234)
    tot = sl_b.batch(sr, hr, caps)
    torch.cuda.synchronize()
    assert per.shape == (B,) and float(per.min()) > 0
    assert torch.equal(per, sl_b.last_per_sample), (per, sl_b.last_per_sample)
    assert abs(float(ts.clip_loss) - float(tot) * lam) <= 1e-6 * float(tot) * lam
    assert torch.equal(loss, ts.l1_loss + ts.clip_loss) and torch.equal(ts.loss, loss)
    ts.all_reduce_grads()
    ts.optimizer_step()
    torch.cuda.synchronize()
    assert ts.micro_count == 0 and bool(torch.isfinite(m_a.flat_params).all())


def test_semantic_differentiable_route_accumulates_the_ordered_sum():
    """differentiable=True: the accumulated gradient of a 2 x 2 cycle equals g_0 + g_1 (torch), g_i the gradient of the route as
    it is without accumulation -- m2t_forward, the encoder's value and gradient, m2t_l1_loss with the CYCLE's divisor,
    m2t_add_output_grad, m2t_backward into a fresh buffer -- under the same torch.manual_seed."""
    from m2trans_amd import _lib
    from m2trans_amd.train_step import TrainStep
    lib = _lib.load()
    scale, nb, B, k, H, W = 4, 4, 4, 2, 128, 128
    b, lam = B // k, 0.01
    caps = [f"c{i}" for i in range(B)]
    m_a, m_b, _ = _twins(scale, nb, "bf16")
    sl_a, sl_b = _semantic(True, b, caps), _semantic(True, b, caps)
    ts = TrainStep(m_a, lr=LR, world_size=1, semantic_loss=sl_a, lambda_clip=lam, accum_steps=k)
    x, hr = _batch(B, H, W, scale, 1)
    torch.manual_seed(99)
    loss = ts.step(x, hr, caps).clone()
    torch.cuda.synchronize()
    grads_a, l1_a, clip_a = ts.grads.clone(), ts.l1_loss.clone(), ts.clip_loss.clone()

    torch.manual_seed(99)
    gsum, l1, clip = None, None, None
    for i in range(k):
        cx, chr_ = x[i * b:(i + 1) * b].contiguous(), hr[i * b:(i + 1) * b].contiguous()
        plan = m_b._plan_for(cx)
        plan.gen += 1
        sr = torch.empty_like(chr_)
        g = torch.full_like(m_b.flat_params, float("nan"))
        li = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
        ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
        _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(m_b.flat_params), _lib.ptr(cx), _lib.ptr(sr), 1.0, 1, ws, st), "m2t_forward")
        tot, gs, origins = sl_b._value_and_grad(sr, chr_, caps[i * b:(i + 1) * b])
        _lib.check(lib.m2t_l1_loss(plan.handle, _lib.ptr(chr_), 1.0, float(hr.numel()), 1.0, _lib.ptr(li), ws, st), "m2t_l1_loss")
        gs = gs.contiguous()
        arr = (C.c_int * (2 * len(origins)))(*[int(v) for o in origins for v in o])
        _lib.check(lib.m2t_add_output_grad(plan.handle, _lib.ptr(gs), gs.shape[2], gs.shape[3], arr, lam, 1.0, ws, st), "m2t_add_output_grad")
        _lib.check(lib.m2t_backward(plan.handle, _lib.ptr(m_b.flat_params), _lib.ptr(cx), _lib.ptr(g), ws, st), "m2t_backward")
        ci = tot * lam
        gsum, l1, clip = (g, li, ci) if gsum is None else (gsum + g, l1 + li, clip + ci)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads_a).all()) and float(clip_a) > 0
    assert torch.equal(l1_a, l1) and torch.equal(clip_a, clip) and torch.equal(loss, l1 + clip)
    assert_flat_equal(m_a, grads_a, gsum, "differentiable SemanticLoss, accumulated gradient vs g_0 + g_1")


# ------------------------------------------------------------------ 10. what must raise
def test_cycle_rule_refusals_change_nothing():
    """k > 1: a batch that k does not divide, optimizer_step / all_reduce_grads / export_checkpoint in the middle of a cycle and a
    forward_backward beyond the k-th raise M2TError BEFORE anything is enqueued or any state changes: completing (for the bad
    batch: running) the cycle afterwards gives the bits of the entry points driven by hand."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.checkpoint import export_checkpoint
    from m2trans_amd.train_step import TrainStep
    scale, nb, H, W = 4, 2, 32, 32
    # a batch of 6 with k = 4
    m_a, m_b, _ = _twins(scale, nb, "fp32")
    ts, ref = TrainStep(m_a, lr=LR, world_size=1, accum_steps=4), _ByHand(m_b)
    before = m_a.flat_params.clone()
    x6, hr6 = _batch(6, H, W, scale, 3)
    with pytest.raises(M2TError, match=r"6.*4"):
        ts.step(x6, hr6)
    torch.cuda.synchronize()
    assert ts.micro_count == 0 and ts.step_count == 0 and torch.equal(m_a.flat_params, before) and len(m_a._plans) == 0
    x, hr = _batch(8, H, W, scale, 1)
    la, lb = ts.step(x, hr).clone(), ref.step(x, hr, 4)
    _compare("a cycle after the refused batch of 6", ts, ref, la, lb)

    # k = 2, driven through forward_backward
    m_a, m_b, _ = _twins(scale, nb, "fp32")
    ts, ref = TrainStep(m_a, lr=LR, world_size=1, accum_steps=2), _ByHand(m_b)
    before = m_a.flat_params.clone()
    x, hr = _batch(4, H, W, scale, 2)
    ts.forward_backward(x[:2], hr[:2])
    torch.cuda.synchronize()
    g_mid, l_mid = ts.grads.clone(), ts.l1_loss.clone()
    for what in (ts.optimizer_step, ts.all_reduce_grads, lambda: export_checkpoint(m_a, ts), lambda: ts.step(x, hr)):
        with pytest.raises(M2TError, match="1 of 2"):
            what()
    torch.cuda.synchronize()
    assert ts.micro_count == 1 and ts.step_count == 0 and torch.equal(m_a.flat_params, before)
    assert torch.equal(ts.grads, g_mid) and torch.equal(ts.l1_loss, l_mid) and float(ts.exp_avg.abs().max()) == 0
    la = ts.forward_backward(x[2:], hr[2:])
    with pytest.raises(M2TError, match="accum_steps"):
        ts.forward_backward(x[:2], hr[:2])                  # a third micro-batch in a k = 2 cycle
    assert ts.micro_count == 2
    la = la.clone()
    ts.all_reduce_grads()
    ts.optimizer_step()
    assert ts.micro_count == 0 and ts.step_count == 1
    lb = ref.step(x, hr, 2)
    _compare("the cycle completed after the refusals", ts, ref, la, lb)
    assert "optimizer_state_dict" in export_checkpoint(m_a, ts)      # between cycles the export works

    # k = 1: repeated forward_backward calls without an optimizer step stay legal and overwrite
    m_c, _ = build_model(scale, nb, "fp32")
    t1 = TrainStep(m_c, lr=LR, world_size=1)
    t1.forward_backward(x[:2], hr[:2])
    l2 = t1.forward_backward(x[2:], hr[2:]).clone()
    torch.cuda.synchronize()
    l_ref, g_ref = _ByHand(m_c).chunk(x[2:], hr[2:], float(hr[2:].numel()))
    torch.cuda.synchronize()
    assert torch.equal(l2, l_ref)
    assert_flat_equal(m_c, t1.grads, g_ref, "accum_steps=1: the second forward_backward overwrites the first")
    assert "optimizer_state_dict" in export_checkpoint(m_c, t1)
