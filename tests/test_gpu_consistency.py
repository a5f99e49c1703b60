"""-m gpu: LR-consistency (k_consistency.hip; include/m2t_consistency.h) against the fp64 restatement tests/consistency_ref.py: the
plan-free loss per element, the all-black pair, the adjoint alone, back-projection one iteration at a time, TrainStep against the
sequence composed by hand, and the Python surface (losses.ConsistencyLoss under autograd through the real model, metrics.lr_psnr_device,
metrics.evaluate_with_lr_psnr, infer.back_project, the command line).

The gate of a gradient or updated element is the restatement's own, 2^-23 |ref| + 2^-40 * coef * (|A_H|^T |g| |A_W|): one fp32
rounding with a factor 2, plus the fp64 reordering of at most 16 x 16 products with a wide margin.  EVERY element is gated.  Values are
gated at 1.2e-7 relative (one fp32 rounding), statistics at 1e-12 relative (sums of non-negative terms).  For eps = 0 the restatement's
min |r| >= 1e-9 is asserted, so that sign(r) is about the kernel and not about conditioning.

LR sizes: 1 x 1 (the halo folds several times), 2 x 3, 5 x 7, 16 x 32 (exactly one forward tile), 17 x 33 (one cell past it), 40 x 56
(several tiles of every kernel at x2 .. x4)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import consistency_ref as CR
from tests.gpu_util import assert_flat_equal

pytestmark = pytest.mark.gpu

ARG = -2
LAM = 0.1
LAM32 = float(torch.tensor(LAM, dtype=torch.float32))              # the weight as the C ABI carries it (a float)
NB = 1


def _lib_():
    from m2trans_amd import _lib
    return _lib, _lib.load()


def _scratch(lib, B, C, H, W, s, poison=False):
    n = lib.m2t_consistency_scratch_bytes(B, C, H, W, s)
    assert n > 0
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    if poison:
        t.fill_(0xFF)                                               # every double a NaN
    return t


def _ratio(got, ref, gate):
    """(elements beyond the gate, largest |got - ref| / gate) for fp64 arrays; a zero gate demands equality."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    ratio = np.where(gate > 0, err / np.maximum(gate, 1e-300), np.where(err > 0, np.inf, 0.0))
    return int((err > gate).sum()), float(ratio.max())


_REF = {}


def _loss_case(s, h, w, C, eps):
    key = (s, h, w, C, eps)
    if key not in _REF:
        x, y = CR.loss_case(s, h, w, C)
        scale = 0.37 / y.size
        _REF[key] = (x, y, scale, CR.loss_ref(x, y, s, 1.0, True, eps, scale))
    return _REF[key]


def _strided(x, pad_rows=2, pad_cols=3, fill=float("nan")):
    """x [B,C,Hs,Ws] inside a `fill`-filled buffer [B,C,Hs + pad_rows,Ws + pad_cols]: (buffer, image stride, row stride)."""
    B, C, Hs, Ws = x.shape
    buf = torch.full((B, C, Hs + pad_rows, Ws + pad_cols), fill, dtype=torch.float32)
    buf[..., :Hs, :Ws] = torch.from_numpy(x) if isinstance(x, np.ndarray) else x
    return buf, C * (Hs + pad_rows) * (Ws + pad_cols), Ws + pad_cols


def _loss_call(lib, _lib, xd, yd, B, C, h, w, s, xs_img, xs_row, clamp, eps, scale, gx, loss, stats, acc, scratch, R=1.0):
    rc = lib.m2t_consistency_loss_tensor(_lib.ptr(xd), _lib.ptr(yd), B, C, h, w, s, xs_img, xs_row, R, clamp, eps, scale, _lib.ptr(gx),
                                         _lib.ptr(loss), _lib.ptr(stats), acc, _lib.ptr(scratch), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------ 1. the plan-free loss against fp64
@pytest.mark.parametrize("hw", CR.LR_SHAPES, ids=[f"{h}x{w}" for h, w in CR.LR_SHAPES])
@pytest.mark.parametrize("s", CR.SCALES)
def test_plan_free_loss_value_gradient_and_statistics_against_fp64(s, hw):
    """C in {1, 3}, eps in {0, 1e-3}, B = 2, the clamp on with values below 0, above R and exactly at both ends; x sits in a NaN-filled
    buffer with a longer row and a padded image stride.  Zero seed: every element within the gate; random seed: the bits of
    fp32(seed + zero-seed result); accumulate on the value; nothing outside [Hs, Ws] touched; two runs and a NaN-filled scratch give
    the same bits; value only gives the same value."""
    _lib, lib = _lib_()
    h, w = hw
    for C in (1, 3):
        for eps in (0.0, 1e-3):
            x, y, scale, ref = _loss_case(s, h, w, C, eps)
            tag = f"x{s} {h}x{w} C{C} eps {eps:g}"
            if eps == 0.0:
                assert ref["min_abs_r"] >= 1e-9, (tag, ref["min_abs_r"])
            assert (x == 0).any() and (x == 1).any(), tag
            if x.size >= 200:
                assert (x < 0).any() and (x > 1).any(), tag
            B, Hs, Ws = x.shape[0], h * s, w * s
            buf, xs_img, xs_row = _strided(x)
            xd, yd = buf.cuda(), torch.from_numpy(y).cuda()
            inside = torch.zeros(buf.shape, dtype=torch.bool)
            inside[..., :Hs, :Ws] = True

            def run(seed, loss0, acc, scratch, with_grad=True, with_stats=True):
                gx = seed.cuda() if with_grad else None
                loss = torch.full((1,), loss0, device="cuda")
                stats = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda") if with_stats else None
                assert _loss_call(lib, _lib, xd, yd, B, C, h, w, s, xs_img, xs_row, 1, eps, scale, gx, loss, stats, acc, scratch) == 0, tag
                return (gx.cpu() if with_grad else None), loss.cpu(), (stats.cpu() if with_stats else None)

            zero = torch.zeros(buf.shape)
            g0, l0, s0 = run(zero, float("nan"), 0, _scratch(lib, B, C, h, w, s))
            got = g0[..., :Hs, :Ws].double().numpy()
            nbad, worst = _ratio(got, ref["grad"], ref["gate"])
            print(f"{tag}: largest |got - ref| / gate {worst:.3f}; value {float(l0):.9e} against {ref['value']:.9e}")
            assert nbad == 0, f"{tag}: {nbad} gradient elements beyond the gate, worst ratio {worst:.3f}"
            assert int(torch.count_nonzero(g0[~inside])) == 0, tag
            assert np.count_nonzero(got[ref["mask"] == 0]) == 0, f"{tag}: gradient where the clamp is active"
            assert abs(float(l0) - ref["value"]) <= 1.2e-7 * abs(ref["value"]), (tag, float(l0), ref["value"])
            assert np.all(np.abs(s0.numpy() - ref["stats"]) <= 1e-12 * ref["stats"]), (tag, s0.tolist(), ref["stats"].tolist())
            # two runs, and a NaN-filled scratch: the same bits
            for poison in (False, True):
                g1, l1, s1 = run(zero, float("nan"), 0, _scratch(lib, B, C, h, w, s, poison))
                assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)) and torch.equal(l1, l0) and torch.equal(s1, s0), (tag, poison)
            # value only
            _, lv, sv = run(None, float("nan"), 0, _scratch(lib, B, C, h, w, s), with_grad=False)
            assert torch.equal(lv, l0) and torch.equal(sv, s0), tag
            _, lv, _ = run(None, float("nan"), 0, _scratch(lib, B, C, h, w, s), with_grad=False, with_stats=False)
            assert torch.equal(lv, l0), tag
            # a random seed is added to with one fp32 add; accumulate adds to the value; the padding keeps its bits
            seed = torch.randn(buf.shape, generator=torch.Generator().manual_seed(3))
            seed[~inside] = float("nan")
            g2, l2, _ = run(seed, 2.5, 1, _scratch(lib, B, C, h, w, s))
            assert torch.equal(g2[..., :Hs, :Ws], seed[..., :Hs, :Ws] + g0[..., :Hs, :Ws]), tag
            assert torch.equal(g2.view(torch.int32)[~inside], seed.view(torch.int32)[~inside]), tag
            assert torch.equal(l2, torch.tensor([2.5]) + l0), (tag, float(l2), float(l0))
            masked = torch.from_numpy(ref["mask"] == 0)
            assert torch.equal(g2[..., :Hs, :Ws].contiguous().view(torch.int32)[masked],
                               seed[..., :Hs, :Ws].contiguous().view(torch.int32)[masked]), tag


def test_clamp_off_and_a_data_range_of_255():
    """The mask applies only with the clamp on; R = 255 scales the residual and the gradient."""
    _lib, lib = _lib_()
    s, h, w, C, R = 3, 5, 7, 3, 255.0
    x, y = CR.loss_case(s, h, w, C, R)
    B = x.shape[0]
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for clamp in (0, 1):
        scale = 1.0 / y.size
        ref = CR.loss_ref(x, y, s, R, bool(clamp), 1e-3, scale)
        gx, loss = torch.zeros_like(xd), torch.zeros(1, device="cuda")
        assert _loss_call(lib, _lib, xd, yd, B, C, h, w, s, C * h * s * w * s, w * s, clamp, 1e-3, scale, gx, loss, None, 0,
                          _scratch(lib, B, C, h, w, s), R=R) == 0
        nbad, worst = _ratio(gx.cpu().double().numpy(), ref["grad"], ref["gate"])
        assert nbad == 0, (clamp, nbad, worst)
        assert abs(float(loss.detach()) - ref["value"]) <= 1.2e-7 * ref["value"]
        if not clamp:
            assert np.count_nonzero(gx.cpu().numpy()[(x < 0) | (x > R)]) > 0


@pytest.mark.parametrize("s", CR.SCALES)
def test_all_black_pair_gives_exactly_zero_and_leaves_the_seed(s):
    """x = 0, y = 0 (the black sector): value exactly 0, sign(0) = 0, the seed numerically unchanged."""
    _lib, lib = _lib_()
    B, C, h, w = 2, 3, 17, 33
    xd, yd = torch.zeros(B, C, h * s, w * s, device="cuda"), torch.zeros(B, C, h, w, device="cuda")
    seed = torch.randn(B, C, h * s, w * s, generator=torch.Generator().manual_seed(1))
    for eps in (0.0, 1e-3):
        gx, loss = seed.cuda(), torch.full((1,), float("nan"), device="cuda")
        stats = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        assert _loss_call(lib, _lib, xd, yd, B, C, h, w, s, C * h * s * w * s, w * s, 1, eps, 1.0 / yd.numel(), gx, loss, stats, 0,
                          _scratch(lib, B, C, h, w, s, True)) == 0
        assert torch.equal(gx.cpu(), seed) and stats.cpu().tolist() == [0.0, 0.0, 0.0]
        if eps == 0.0:
            assert float(loss) == 0.0
        else:
            assert abs(float(loss) - eps) <= 1.2e-7 * eps               # rho(0) = eps


def test_entry_points_refuse_bad_arguments_before_any_launch():
    _lib, lib = _lib_()
    B, C, h, w, s = 1, 3, 4, 4, 2
    x, y = torch.zeros(B, C, 8, 8, device="cuda"), torch.zeros(B, C, h, w, device="cuda")
    gx, loss, scratch = torch.ones_like(x), torch.full((1,), 7.0, device="cuda"), _scratch(lib, B, C, h, w, s)
    base = dict(x=x, y=y, B=B, C=C, H=h, W=w, s=s, img=C * 64, row=8, R=1.0, clamp=1, eps=0.0, scale=1.0, gx=gx, loss=loss, scratch=scratch)
    for bad in (dict(x=None), dict(y=None), dict(loss=None), dict(scratch=None), dict(s=1), dict(s=5), dict(C=2, img=128), dict(H=0), dict(W=0),
                dict(H=8193), dict(row=7), dict(img=C * 64 - 3), dict(R=0.0), dict(R=float("nan")), dict(eps=-1.0), dict(eps=float("inf")),
                dict(scale=float("nan")), dict(B=0), dict(B=21846)):
        a = dict(base)
        a.update(bad)
        rc = lib.m2t_consistency_loss_tensor(_lib.ptr(a["x"]), _lib.ptr(a["y"]), a["B"], a["C"], a["H"], a["W"], a["s"], a["img"], a["row"],
                                             a["R"], a["clamp"], a["eps"], a["scale"], _lib.ptr(a["gx"]), _lib.ptr(a["loss"]), None, 0,
                                             _lib.ptr(a["scratch"]), _lib.stream_ptr())
        assert rc == ARG, bad
    sr = torch.rand(B, C, 8, 8, device="cuda")
    bits = sr.clone()
    for beta in (2.0, 0.0, -0.5, float("nan"), float("inf")):
        assert lib.m2t_back_project_f32(_lib.ptr(sr), _lib.ptr(y), B, C, h, w, s, 1.0, beta, 1, None, _lib.ptr(scratch), _lib.stream_ptr()) == ARG
    assert b"beta" in lib.m2t_last_error_string()
    assert lib.m2t_back_project_f32(None, _lib.ptr(y), B, C, h, w, s, 1.0, 1.0, 1, None, _lib.ptr(scratch), _lib.stream_ptr()) == ARG
    assert lib.m2t_imresize_adjoint_f32(_lib.ptr(y), 3, h, w, _lib.ptr(sr), 5, 0, _lib.stream_ptr()) == ARG
    assert lib.m2t_imresize_adjoint_f32(None, 3, h, w, _lib.ptr(sr), 2, 0, _lib.stream_ptr()) == ARG
    torch.cuda.synchronize()
    assert torch.equal(sr, bits) and float(loss) == 7.0 and torch.equal(gx, torch.ones_like(gx))        # a refused call touches nothing
    assert lib.m2t_consistency_scratch_bytes(1, 2, 4, 4, 2) == 0 and lib.m2t_consistency_scratch_bytes(1, 3, 4, 4, 5) == 0
    assert lib.m2t_consistency_scratch_bytes(2, 3, 17, 33, 4) == 8 * (2 * 3 * 17 * 33 + 2 * 3 * 2 * 2 * 4)


# ------------------------------------------------------------------ 2. the adjoint alone
@pytest.mark.parametrize("hw", CR.LR_SHAPES, ids=[f"{h}x{w}" for h, w in CR.LR_SHAPES])
@pytest.mark.parametrize("s", CR.SCALES)
def test_imresize_adjoint_against_the_dense_form_and_the_dot_product_identity(s, hw):
    from m2trans_amd import resize
    _lib, lib = _lib_()
    h, w = hw
    rng = np.random.default_rng(50 + s)
    g = rng.standard_normal((2, 3, h, w)).astype(np.float32)
    gd = torch.from_numpy(g).cuda()
    got = resize.imresize_adjoint(gd, s)
    ref = CR.adjoint(g, s)
    gate = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * CR.adjoint_abs(g, s)
    nbad, worst = _ratio(got.cpu().double().numpy(), ref, gate)
    assert nbad == 0, (nbad, worst)
    # accumulate != 0 adds with one fp32 add
    out = torch.full_like(got, 0.5)
    _lib.check(lib.m2t_imresize_adjoint_f32(_lib.ptr(gd), 6, h, w, _lib.ptr(out), s, 1, _lib.stream_ptr()), "m2t_imresize_adjoint_f32")
    assert torch.equal(out, torch.full_like(got, 0.5) + got)
    # <D x, g> = <x, D^T g> with the device's own down-sampler
    x = torch.from_numpy(rng.standard_normal((2, 3, h * s, w * s)).astype(np.float32)).cuda()
    lhs = float((resize.imresize(x, s).double() * gd.double()).sum())
    rhs = float((x.double() * got.double()).sum())
    size = float((resize.imresize(x, s).double() * gd.double()).abs().sum())
    assert abs(lhs - rhs) <= 1e-6 * size, (lhs, rhs, size)


# ------------------------------------------------------------------ 3. back-projection
def _bp_call(lib, _lib, sr, lr, s, beta, update, stats, scratch, R=1.0):
    B, C, h, w = lr.shape
    rc = lib.m2t_back_project_f32(_lib.ptr(sr), _lib.ptr(lr), B, C, h, w, s, R, beta, update, _lib.ptr(stats), _lib.ptr(scratch),
                                  _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("beta", [0.5, 1.0, 1.5])
@pytest.mark.parametrize("case", CR.BP_CASES, ids=[f"x{c[0]}-{c[1]}x{c[2]}-C{c[3]}{'-clamp' if c[4] else ''}" for c in CR.BP_CASES])
def test_back_projection_one_iteration_at_a_time_against_fp64(case, beta):
    """Four iterations, teacher-forced from the device's own previous output: every updated element within the gate, the statistics (the
    state BEFORE the update) at 1e-12; update = 0 leaves sr's bits; infer.back_project's statistics tensor equals the per-call values."""
    from m2trans_amd import infer
    _lib, lib = _lib_()
    s, h, w, C, clamp_active = case
    sr0, lr = CR.bp_case(s, h, w, C, clamp_active=clamp_active)
    B = lr.shape[0]
    lrd, cur = torch.from_numpy(lr).cuda(), torch.from_numpy(sr0).cuda()
    rows, hit = [], 0
    for it in range(4):
        before = cur.cpu().numpy()
        ref = CR.back_project_ref(before, lr, s, 1.0, beta)
        stats = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        probe = cur.clone()
        assert _bp_call(lib, _lib, probe, lrd, s, beta, 0, stats, _scratch(lib, B, C, h, w, s, True)) == 0
        assert torch.equal(probe.view(torch.int32), cur.view(torch.int32))                       # update = 0: the bits stay
        stats2 = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        assert _bp_call(lib, _lib, cur, lrd, s, beta, 1, stats2, _scratch(lib, B, C, h, w, s)) == 0
        assert torch.equal(stats, stats2)
        assert np.all(np.abs(stats.cpu().numpy() - ref["stats"]) <= 1e-12 * ref["stats"]), (it, stats.tolist(), ref["stats"].tolist())
        nbad, worst = _ratio(cur.cpu().double().numpy(), ref["new"], ref["gate"])
        assert nbad == 0, f"iteration {it}: {nbad} elements beyond the gate, worst ratio {worst:.3f}"
        hit += int(((ref["pre"] < 0) | (ref["pre"] > 1)).sum())
        rows.append(stats.cpu())
    assert float(cur.min()) >= 0.0 and float(cur.max()) <= 1.0
    if clamp_active:
        assert hit > 0, "the clamp was meant to be active"
    out, table = infer.back_project(torch.from_numpy(sr0).cuda(), lrd, s, iters=4, beta=beta, with_stats=True)
    torch.cuda.synchronize()
    assert torch.equal(out, cur) and tuple(table.shape) == (5, 3)
    assert torch.equal(table[:4].cpu(), torch.stack(rows))
    last = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    assert _bp_call(lib, _lib, cur.clone(), lrd, s, beta, 0, last, _scratch(lib, B, C, h, w, s)) == 0
    assert torch.equal(table[4], last)
    assert torch.equal(infer.back_project(torch.from_numpy(sr0).cuda(), lrd, s, iters=4, beta=beta), out)
    if case in CR.BP_MONOTONE and beta == 1.0:                          # (checked on the CPU for these inputs)
        mx = table[:, 1].cpu().tolist()
        assert all(b < a for a, b in zip(mx, mx[1:])), mx


# ------------------------------------------------------------------ 4. TrainStep against the sequence by hand
def _step_helpers():
    from tests.test_gpu_msssim_loss import _model, _pair, _pixel, _srpre
    from tests.test_gpu_pixel_loss import _backward, _forward
    return _model, _pair, _pixel, _srpre, _backward, _forward


def _by_hand(model, plan, x, hr, lam=LAM32, eps=0.0, pix_div=None, cons_div=None, more=None):
    """(l1 [1], consistency [1], gradients): m2t_forward -> m2t_pixel_loss (l1) -> [more] -> the PLAN-FREE entry on the forward's own
    pre-clamp output, adding into the seed in the workspace -> m2t_backward, into fresh buffers."""
    _model, _pair, _pixel, _srpre, _backward, _forward = _step_helpers()
    _lib, lib = _lib_()
    B, _, H, W = x.shape
    s = model.scale
    l1, co = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    grads = torch.full_like(model.flat_params, float("nan"))
    _forward(lib, model, plan, x)
    assert _pixel(lib, plan, hr, l1, divisor=pix_div) == 0
    if more is not None:
        more(lib, plan, hr)
    pre = _srpre(plan, B, s)
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    Hp, Wp = pre.shape[-2:]
    div = float(x.numel() if cons_div is None else cons_div)
    scratch = _scratch(lib, B, 3, H, W, s)
    assert _loss_call(lib, _lib, pre, x, B, 3, H, W, s, 3 * Hp * Wp, Wp, 1, eps, lam / div, gpre, co, None, 0, scratch) == 0
    _backward(lib, model, plan, x, grads)
    torch.cuda.synchronize()
    return l1, co, grads


@pytest.mark.parametrize("dtype,scale,eps", [("bf16", 4, 0.0), ("fp32", 2, 1e-3)])
def test_train_step_is_the_sequence_by_hand(dtype, scale, eps):
    """Two steps at (2, 20, 28): consistency_loss equals the plan-free entry on the step's own forward output bit for bit, and the
    gradients, parameters and moments equal those of a twin given the summed seed by hand; the term is live."""
    from m2trans_amd.train_step import TrainStep
    _model, _pair, _pixel, _srpre, _backward, _forward = _step_helpers()
    _lib, lib = _lib_()
    B, H, W = 2, 20, 28
    m_a, m_b = _model(scale, dtype, NB), _model(scale, dtype, NB)
    ts = TrainStep(m_a, lr=1e-4, world_size=1, lambda_consistency=LAM, consistency_eps=eps)
    exp_avg, exp_avg_sq = torch.zeros_like(m_b.flat_params), torch.zeros_like(m_b.flat_params)
    first_grads = None
    for step in range(2):
        x, hr = _pair(scale, dtype, B, H, W, step)
        loss = ts.step(x, hr)
        torch.cuda.synchronize()
        l1, co, grads = _by_hand(m_b, m_b._plan_for(x), x, hr, eps=eps)
        if step == 0:
            first_grads = grads.clone()
        _lib.check(lib.m2t_adam_step(_lib.ptr(m_b.flat_params), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), grads.numel(), 1e-4,
                                     0.9, 0.999, 1e-8, step + 1, 1.0, _lib.stream_ptr()), "m2t_adam_step")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(grads).all()) and 0 < float(co) < LAM and float(l1) > 0
        assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.consistency_loss, co) and torch.equal(loss, l1 + co), (step, float(loss))
        assert list(ts._consistency_scratch) == [(B, H, W)]
        assert_flat_equal(m_a, ts.grads, grads, f"gradients, step {step}")
        assert_flat_equal(m_a, m_a.flat_params.detach(), m_b.flat_params.detach(), f"parameters, step {step}")
        assert_flat_equal(m_a, ts.exp_avg, exp_avg, f"exp_avg, step {step}")
        assert_flat_equal(m_a, ts.exp_avg_sq, exp_avg_sq, f"exp_avg_sq, step {step}")
    x, hr = _pair(scale, dtype, B, H, W, 0)
    ts0 = TrainStep(_model(scale, dtype, NB), world_size=1)
    ts0.forward_backward(x, hr)
    torch.cuda.synchronize()
    assert not torch.equal(ts0.grads, first_grads)


def test_plan_entry_leaves_zero_in_the_reflect_padding():
    """m2t_pixel_loss of weight 0 then m2t_consistency_loss on a reflect-padded shape: the seed is exactly 0 in the padding and where the
    clamp is active, and within the gate of the restatement elsewhere."""
    _model, _pair, _pixel, _srpre, _backward, _forward = _step_helpers()
    _lib, lib = _lib_()
    scale, B, H, W = 3, 1, 21, 27
    model = _model(scale, "fp32", NB)
    x, hr = _pair(scale, "fp32", B, H, W)
    plan = model._plan_for(x)
    _forward(lib, model, plan, x)
    torch.cuda.synchronize()
    pre = _srpre(plan, B, scale).clone()
    Hs, Ws = H * scale, W * scale
    assert tuple(pre.shape[-2:]) != (Hs, Ws), "the shape is meant to be reflect-padded"
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    gpre.fill_(float("nan"))
    l1, out = torch.zeros(1, device="cuda"), torch.full((1,), float("nan"), device="cuda")
    assert _pixel(lib, plan, hr, l1, weight=0.0) == 0
    rc = lib.m2t_consistency_loss(plan.handle, _lib.ptr(x), LAM, float(x.numel()), 1.0, 1e-3, _lib.ptr(out), 0,
                                  _lib.ptr(_scratch(lib, B, 3, H, W, scale)), _lib.ptr(plan.workspace), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    got = gpre.view(pre.shape).double().cpu().numpy()
    inner = pre[..., :Hs, :Ws].cpu().numpy()
    ref = CR.loss_ref(inner, x.cpu().numpy(), scale, 1.0, True, 1e-3, LAM32 / x.numel())
    pad = np.ones(got.shape, dtype=bool)
    pad[..., :Hs, :Ws] = False
    assert np.isfinite(got).all() and np.count_nonzero(got[pad]) == 0
    nbad, worst = _ratio(got[..., :Hs, :Ws], ref["grad"], ref["gate"])
    assert nbad == 0, (nbad, worst)
    assert np.count_nonzero(got[..., :Hs, :Ws][ref["mask"] == 0]) == 0
    assert abs(float(out) - ref["value"]) <= 1.2e-7 * ref["value"]
    # the state rules of m2t_gmsd_loss: a deferred pixel loss leaves no materialised seed
    assert _pixel(lib, plan, hr, l1, deferred=True) == 0
    assert lib.m2t_consistency_loss(plan.handle, _lib.ptr(x), LAM, float(x.numel()), 1.0, 0.0, _lib.ptr(out), 0,
                                    _lib.ptr(_scratch(lib, B, 3, H, W, scale)), _lib.ptr(plan.workspace), _lib.stream_ptr()) == -3


def test_lambda_consistency_zero_is_the_default_step_bit_for_bit(monkeypatch):
    """Weight 0 allocates nothing, makes no call to the new entries, and gives the step of today bit for bit."""
    from m2trans_amd import _lib as L
    from m2trans_amd.train_step import TrainStep
    _model, _pair, _pixel, _srpre, _backward, _forward = _step_helpers()
    scale, dtype, B, H, W = 4, "bf16", 2, 20, 28
    real = L.load()
    called = []

    class Spy:
        def __getattr__(self, name):
            if "consistency" in name or "back_project" in name or "adjoint" in name:
                called.append(name)
            return getattr(real, name)
    res = []
    for kw in ({}, {"lambda_consistency": 0.0, "consistency_eps": 1e-3}):
        model = _model(scale, dtype, NB)
        ts = TrainStep(model, lr=1e-4, world_size=1, **kw)
        assert ts.consistency_loss is None and not ts._consistency_scratch
        out = []
        for step in range(2):
            x, hr = _pair(scale, dtype, B, H, W, step)
            with monkeypatch.context() as mp:
                mp.setattr(L, "load", lambda: Spy())
                loss = ts.step(x, hr)
            torch.cuda.synchronize()
            assert loss is ts.l1_loss and ts.consistency_loss is None
            out.append((loss.clone(), ts.grads.clone(), model.flat_params.detach().clone()))
        res.append((model, out))
    assert called == []
    (model, a), (_, b) = res
    for step in range(2):
        assert torch.equal(a[step][0], b[step][0])
        assert_flat_equal(model, a[step][1], b[step][1], f"gradients, step {step}")
        assert_flat_equal(model, a[step][2], b[step][2], f"parameters, step {step}")


def test_accumulated_consistency_equals_the_micro_batch_shares_summed_in_call_order():
    """accum_steps = 2 at micro-batch (1, 20, 28), bf16 x4: the accumulated buffer is the fp32 sum, in call order, of the two micro-batch
    gradients by hand with the cycle's divisors (the global number of LR elements); ts.consistency_loss is the sum of the two."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    _model, _pair, _pixel, _srpre, _backward, _forward = _step_helpers()
    x, hr = _pair(4, "bf16", 2, 20, 28)
    m_a, m_b = _model(4, "bf16", NB), _model(4, "bf16", NB)
    ts = TrainStep(m_a, world_size=1, accum_steps=2, lambda_consistency=LAM)
    ts.forward_backward(x[0:1], hr[0:1])
    with pytest.raises(M2TError):
        ts.set_lambda_consistency(0.0)
    loss = ts.forward_backward(x[1:2], hr[1:2])
    torch.cuda.synchronize()
    parts = []
    for i in range(2):
        cx, chr_ = x[i:i + 1].contiguous(), hr[i:i + 1].contiguous()
        parts.append(_by_hand(m_b, m_b._plan_for(cx), cx, chr_, pix_div=hr.numel(), cons_div=x.numel()))
    assert float(parts[1][1]) > 0
    assert torch.equal(ts.consistency_loss, parts[0][1] + parts[1][1])
    assert torch.equal(ts.l1_loss, parts[0][0] + parts[1][0]) and torch.equal(loss, ts.l1_loss + ts.consistency_loss)
    assert_flat_equal(m_a, ts.grads, parts[0][2] + parts[1][2], "accumulated L1 + consistency")
    ts.optimizer_step()
    assert ts.micro_count == 0


def test_the_term_runs_with_lambda_ssim_and_with_param_groups():
    """pixel -> SSIM -> consistency -> backward equals that sequence by hand bit for bit; with the head and body frozen the step runs,
    the frozen tensors keep their bits and the tail moves."""
    from m2trans_amd import _lib as L
    from m2trans_amd.train_step import TrainStep
    _model, _pair, _pixel, _srpre, _backward, _forward = _step_helpers()
    scale, dtype, B, H, W = 4, "bf16", 2, 20, 28
    x, hr = _pair(scale, dtype, B, H, W)
    m_a, m_b = _model(scale, dtype, NB), _model(scale, dtype, NB)
    ts = TrainStep(m_a, world_size=1, lambda_ssim=0.1, lambda_consistency=LAM)
    loss = ts.forward_backward(x, hr)
    torch.cuda.synchronize()
    ss = torch.full((1,), float("nan"), device="cuda")

    def ssim(lib, plan, hr_):
        n = lib.m2t_ssim_loss_scratch_bytes(B, 3, H * scale, W * scale)
        scratch = torch.empty(n, dtype=torch.uint8, device="cuda")
        div = float(B * 3 * (H * scale - 10) * (W * scale - 10))
        assert lib.m2t_ssim_loss(plan.handle, L.ptr(hr_), 0.1, div, 1.0, L.ptr(ss), 0, L.ptr(scratch), L.ptr(plan.workspace), L.stream_ptr()) == 0
        torch.cuda.synchronize()
    l1, co, grads = _by_hand(m_b, m_b._plan_for(x), x, hr, more=ssim)
    assert torch.equal(ts.ssim_loss, ss) and torch.equal(ts.consistency_loss, co) and torch.equal(loss, l1 + ss + co)
    assert_flat_equal(m_a, ts.grads, grads, "pixel + SSIM + consistency")
    m_c = _model(scale, dtype, NB)
    before = m_c.flat_params.detach().clone()
    tg = TrainStep(m_c, lr=1e-4, world_size=1, lambda_consistency=LAM, param_groups=[{"params": ["head", "body"], "frozen": True}])
    tg.step(x, hr)
    torch.cuda.synchronize()
    offs = m_c.param_offsets()
    moved = {n for n, (o, k) in offs.items() if not torch.equal(before[o:o + k], m_c.flat_params.detach()[o:o + k])}
    assert moved and all(n.startswith("tail") for n in moved), sorted(moved)
    assert float(tg.consistency_loss) > 0


# ------------------------------------------------------------------ 5. the Python surface
def test_consistency_loss_fine_tunes_on_lr_alone_through_the_real_model():
    """losses.ConsistencyLoss under autograd through the fp32 model: no HR anywhere; three stock-Adam steps lower the term.  The value
    is the restatement's mean on the model's own output."""
    from m2trans_amd.losses import ConsistencyLoss
    from tests.gpu_util import build_model
    from oracle import m2trans_oracle as O
    scale = 4
    model, _ = build_model(scale, NB, "fp32")
    model.train()
    lr = O.closed_form_image(2, 3, 20, 28, phase=0.3).cuda()
    crit = ConsistencyLoss(scale, eps=1e-3)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    values = []
    for it in range(4):
        opt.zero_grad()
        sr = model(lr)
        loss = crit(sr, lr)
        if it == 0:
            ref = CR.loss_ref(sr.detach().cpu().numpy(), lr.cpu().numpy(), scale, 1.0, True, 1e-3, 1.0 / lr.numel())
            assert abs(float(loss.detach()) - ref["value"]) <= 1.2e-7 * ref["value"]
        values.append(float(loss.detach()))
        if it < 3:
            loss.backward()
            assert all(p.grad is not None for p in model.parameters() if p.requires_grad)
            opt.step()
    print("lr-only fine-tuning, the term over three Adam steps:", values)
    assert values[3] < values[0], values


def test_autograd_gradient_is_the_entrys_gradient_scaled_by_the_upstream_one():
    from m2trans_amd.losses import consistency_loss
    s, h, w, C = 3, 5, 7, 3
    x, y = CR.loss_case(s, h, w, C)
    ref = CR.loss_ref(x, y, s, 1.0, True, 0.0, 1.0 / y.size)
    leaf = torch.from_numpy(x).cuda().requires_grad_(True)
    (2.0 * consistency_loss(leaf, torch.from_numpy(y).cuda(), s)).backward()
    nbad, worst = _ratio(leaf.grad.cpu().double().numpy(), 2.0 * ref["grad"], 2.0 * ref["gate"])
    assert nbad == 0, (nbad, worst)


def test_lr_psnr_metric_and_the_evaluation_entry():
    from m2trans_amd import infer, metrics, resize
    s, h, w = 4, 17, 33
    sr0, lr = CR.bp_case(s, h, w, 3)
    srd, lrd = torch.from_numpy(sr0).cuda(), torch.from_numpy(lr).cuda()
    got = metrics.lr_psnr_device(srd, lrd, s, 1.0)
    want = CR.lr_psnr_ref(sr0, lr, s)
    assert got.dtype == torch.float64 and tuple(got.shape) == (1,) and abs(float(got) - want) <= 1e-9, (float(got), want)
    # evaluate_with_lr_psnr: evaluate's own outputs, then the average LR-PSNR; BackProject composes under it and raises the score
    g = torch.Generator().manual_seed(0)
    pairs = []
    for i in range(2):
        hr = torch.rand(1, 3, 24 * s, 20 * s, generator=g).cuda()
        pairs.append((resize.imresize(hr, s, clamp_max=1.0), hr))
    base = resize.BicubicUp(s)
    plain = metrics.evaluate(base, pairs, s)
    scored = metrics.evaluate_with_lr_psnr(base, pairs, s)
    assert scored[:2] == plain and len(scored) == 3
    each = [float(metrics.lr_psnr_device(base(lr_), lr_, s)) for lr_, _ in pairs]
    assert scored[2] == round(sum(each) / 2 + 5e-3, 2)
    better = metrics.evaluate_with_lr_psnr(infer.BackProject(base, s, iters=3), pairs, s, with_gmsd=True)
    assert len(better) == 4 and better[3] > scored[2], (better, scored)


def test_the_command_line_back_projects_and_writes_consistency_json(tmp_path, capsys):
    """`python -m m2trans_amd.infer --back_project 3` in process on two small images: consistency.json beside the results with LR-PSNR
    after >= before; without the option nothing changes (no file, no keys)."""
    import yaml
    from PIL import Image
    from m2trans_amd import infer
    from tests.test_gpu_infer import _model
    scale = 2
    model = _model(scale, "fp32")
    torch.save({"epoch": 3, "model_state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}}, tmp_path / "m.pt")
    with open(tmp_path / "c.yml", "w") as f:
        yaml.safe_dump({"model": "M2Trans", "scale": scale, "n_blocks": 1, "n_feats": 64, "colors": 3, "rgb_range": 1.0, "compute_dtype": "fp32"}, f)
    (tmp_path / "in").mkdir()
    rng = np.random.default_rng(5)
    for name, (h, w) in {"a.png": (24, 40), "b.png": (33, 21)}.items():
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(tmp_path / "in" / name)
    argv = ["--config", str(tmp_path / "c.yml"), "--model_path", str(tmp_path / "m.pt"), "--input", str(tmp_path / "in"), "--output"]
    assert infer.main(argv + [str(tmp_path / "plain")]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "back_project" not in line and "consistency" not in line and not os.path.exists(tmp_path / "plain" / "consistency.json")
    assert infer.main(argv + [str(tmp_path / "bp"), "--back_project", "3", "--back_project_beta", "1.0"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["back_project"] == 3 and line["back_project_beta"] == 1.0 and line["images"] == 2
    rec = json.load(open(tmp_path / "bp" / "consistency.json"))
    assert rec["iters"] == 3 and set(rec["images"]) == {"a.png", "b.png"}
    for name, r in rec["images"].items():
        assert r["after"]["lr_psnr"] >= r["before"]["lr_psnr"], (name, r)
        lr = infer.load_image(tmp_path / "in" / name, "cuda")
        with torch.no_grad():
            want, stats = infer.back_project(model(lr), lr, scale, 3, 1.0, with_stats=True)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "bp" / name)), infer.to_uint8(want).cpu().numpy())
        assert r["before"]["mean_residual"] == float(stats[0, 0]) and r["after"]["max_residual"] == float(stats[3, 1])
