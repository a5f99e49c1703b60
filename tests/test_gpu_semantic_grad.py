"""-m gpu: the opt-in differentiable SemanticLoss (Swin-T data gradient in HIP) against torch autograd of the fp64 oracle
(oracle/swin_oracle.py) with the image side taken out of no_grad.  The default (non-differentiable) behaviour is pinned by
tests/test_gpu_swin.py and stays as it is."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import swin_oracle as S

pytestmark = pytest.mark.gpu

_P64 = None


def _p64():
    global _P64
    if _P64 is None:
        _P64 = S.closed_form_swin_params(dtype=torch.float64)
    return _P64


def _loss(dt="fp32", n_patches=3, differentiable=True, max_batch=4):
    from m2trans_amd.losses import SemanticLoss
    sl = SemanticLoss(criterion="l1", N_patches=n_patches, device="cuda", compute_dtype=dt, max_batch=max_batch,
                      differentiable=differentiable)
    sl.load_image_encoder(S.closed_form_swin_params())
    return sl


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _cos(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float(a @ b / (a.norm() * b.norm()))


@pytest.mark.parametrize("dt,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_encoder_vjp_matches_fp64_autograd(dt, tol):
    from m2trans_amd import _lib
    sl = _loss(dt)
    enc = sl._encoder()
    g = torch.Generator().manual_seed(11)
    src = torch.rand(2, 3, 256, 272, generator=g)
    crops = [(0, 5, 17), (1, 32, 48), (0, 0, 0)]
    u = torch.randn(3, 512, generator=g)
    # fp64 oracle: d <encode_image(crops), u> / d crops
    leaf = torch.stack([src[i, :, y:y + 224, x:x + 224] for i, y, x in crops]).double().requires_grad_(True)
    want = torch.autograd.grad(S.encode_image(leaf, _p64()), leaf, u.double())[0]
    srcg = src.cuda()
    emb = enc.encode_grad(srcg, None, crops, 3)
    g_crops = enc.backward(u.cuda(), 3)
    torch.cuda.synchronize()
    assert g_crops.shape == (3, 3, 224, 224)
    assert torch.isfinite(g_crops).all()
    err = _rel_l2(g_crops, want)
    assert err <= tol, err
    if dt == "fp32":
        assert torch.equal(emb, enc.encode(srcg, crops)), "grad-mode emb must be bit-identical to encode_pair's in fp32"
    else:
        assert _cos(g_crops, want) >= 0.995
        ref = torch.cat([S.encode_image(src[i:i + 1, :, y:y + 224, x:x + 224], S.closed_form_swin_params()) for i, y, x in crops])
        assert float((emb.cpu() - ref).abs().max() / ref.abs().max()) < 3e-2
    # backward needs a stash of the same crop count
    lib = _lib.load()
    rc = lib.m2t_swin_backward(enc.handle, _lib.ptr(u.cuda()), 2, _lib.ptr(g_crops), _lib.ptr(enc.workspace),
                               _lib.ptr(enc.grad_workspace), _lib.stream_ptr())
    assert rc != 0


@pytest.mark.parametrize("shape", [(256, 240), (200, 180), (300, 190)])
def test_bicubic_backward_is_the_adjoint(shape):
    from m2trans_amd import _lib
    hin, win = shape
    g = torch.Generator().manual_seed(5)
    # fp32 input: torch then forms the source coordinates in fp32 as m2t_bicubic_resize does (an fp64 reference differs from
    # both by ~1e-5 relative through the coordinates alone)
    x = torch.rand(2, 3, hin, win, generator=g, requires_grad=True)
    gd = torch.randn(2, 3, 224, 224, generator=g)
    y = F.interpolate(x, mode="bicubic", size=(224, 224), align_corners=True)
    want = torch.autograd.grad(y, x, gd)[0].double()
    gdg = gd.cuda()
    outs = []
    for _ in range(2):
        out = torch.full((2, 3, hin, win), float("nan"), device="cuda")
        _lib.check(_lib.load().m2t_bicubic_resize_backward(_lib.ptr(gdg), _lib.ptr(out), 6, hin, win, 224, 224, _lib.stream_ptr()),
                   "m2t_bicubic_resize_backward")
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]), "a gather is deterministic"
    err = float((outs[0].double() - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), err


def _oracle_total(sr, hr, table, caps, n_patches):
    """semantic_loss_value with the image side outside no_grad (out-of-place normalisations), fp64, same RNG use."""
    p = _p64()
    tot = 0.0
    for i in range(sr.shape[0]):
        x, y = sr[i:i + 1], hr[i:i + 1]
        px = [F.interpolate(x, mode="bicubic", size=(224, 224), align_corners=True)]
        py = [F.interpolate(y, mode="bicubic", size=(224, 224), align_corners=True)]
        if n_patches > 1:
            for xc, yc in S.draw_patch_coords(x.shape[2], x.shape[3], n_patches):
                px.append(x[:, :, xc:xc + 224, yc:yc + 224])
                py.append(y[:, :, xc:xc + 224, yc:yc + 224])
        xe = S.encode_image(px[-1], p)
        with torch.no_grad():
            ye = S.encode_image(py[-1], p)
        t = table[caps[i]].double()
        t = t / t.norm()
        tot = tot + ((xe @ t) - (ye @ t)).abs().sum() / float(n_patches)
    return tot


@pytest.mark.parametrize("n_patches", [3, 1])
def test_semantic_loss_batch_gradient(n_patches):
    sl = _loss("fp32", n_patches)
    ref_sl = _loss("fp32", n_patches, differentiable=False)
    g = torch.Generator().manual_seed(4)
    B = 3
    sr = torch.rand(B, 3, 256, 240, generator=g)
    hr = torch.rand(B, 3, 256, 240, generator=g)
    caps = ["thyroid nodule, transverse", "carotid artery long axis", "liver segment"]
    table = {c: torch.randn(512, generator=g) for c in caps}
    sl.set_text_features(table)
    ref_sl.set_text_features(table)
    # value and RNG consumption identical to the default mode
    torch.manual_seed(33)
    want_tot = ref_sl.batch(sr.cuda(), hr.cuda(), caps)
    after_ref = torch.get_rng_state()
    torch.manual_seed(33)
    srg = sr.cuda().requires_grad_(True)
    tot = sl.batch(srg, hr.cuda(), caps)
    assert torch.equal(torch.get_rng_state(), after_ref)
    assert torch.equal(tot.detach(), want_tot)
    assert tot.requires_grad
    tot.backward()
    got = srg.grad.clone()
    # fp64 oracle with the same crops
    torch.manual_seed(33)
    last = [S.draw_patch_coords(256, 240, n_patches)[-1] if n_patches > 1 else None for _ in range(B)]
    torch.manual_seed(33)
    x64 = sr.double().requires_grad_(True)
    ref = _oracle_total(x64, hr.double(), table, caps, n_patches)
    want = torch.autograd.grad(ref, x64)[0]
    assert abs(float(ref) - float(want_tot)) < 5e-5
    err = _rel_l2(got, want)
    assert err <= 1e-3, err
    if n_patches > 1:
        for i, (y0, x0) in enumerate(last):
            mask = torch.ones(3, 256, 240, dtype=torch.bool)
            mask[:, y0:y0 + 224, x0:x0 + 224] = False
            assert torch.count_nonzero(got[i].cpu()[mask]) == 0, "gradient outside the last crop"
    # scaling by the upstream gradient
    torch.manual_seed(33)
    srg2 = sr.cuda().requires_grad_(True)
    (2.5 * sl.batch(srg2, hr.cuda(), caps)).backward()
    assert _rel_l2(srg2.grad, 2.5 * got) < 1e-6
    # the per-sample call surface (train.py:205) gives sample 0's gradient
    torch.manual_seed(33)
    s0 = sr[0].cuda().requires_grad_(True)
    one = sl(s0, hr[0].cuda(), caps[0])
    one.backward()
    assert _rel_l2(s0.grad, got[0]) < 1e-5
    # a second call before backward does not disturb the first (no stash lives across calls)
    torch.manual_seed(33)
    a = sr.cuda().requires_grad_(True)
    ta = sl.batch(a, hr.cuda(), caps)
    torch.manual_seed(34)
    sl.batch(hr.cuda().requires_grad_(True), sr.cuda(), caps)
    ta.backward()
    assert torch.equal(a.grad, got)


def _model_and_inputs(dt):
    from oracle import m2trans_oracle as O
    from tests.gpu_util import build_model
    scale, nb, B, H, W = 4, 1, 2, 64, 64
    model, _ = build_model(scale, nb, dt)
    x = O.closed_form_image(B, 3, H, W).cuda()
    hr = O.closed_form_image(B, 3, H * scale, W * scale, phase=0.7).cuda()
    return model, x, hr


@pytest.mark.parametrize("dt,tol", [("fp32", 1e-5), ("bf16", 1e-2)])
def test_train_step_with_differentiable_semantic_loss(dt, tol):
    from m2trans_amd.train_step import TrainStep
    model, x, hr = _model_and_inputs(dt)
    sl = _loss(dt, 3)
    g = torch.Generator().manual_seed(8)
    sl.set_text_features({"a": torch.randn(512, generator=g), "b": torch.randn(512, generator=g)})
    caps = ["a", "b"]
    ts0 = TrainStep(model, world_size=1)
    ts0.forward_backward(x, hr)
    g_l1 = ts0.grads.clone()
    ts = TrainStep(model, world_size=1, semantic_loss=sl, lambda_clip=0.01)
    torch.manual_seed(1)
    loss = ts.forward_backward(x, hr, caps)
    torch.cuda.synchronize()
    g_fast = ts.grads.clone()
    per = sl.last_per_sample.clone()
    assert abs(float(loss) - (float(ts.l1_loss) + 0.01 * float(per.sum()))) < 1e-6
    # the autograd route
    for prm in model.parameters():
        prm.grad = None
    torch.manual_seed(1)
    sr = model(x)
    tot = sl.batch(sr, hr, caps)
    (F.l1_loss(sr, hr) + 0.01 * tot).backward()
    offs = model.param_offsets()
    named = dict(model.named_parameters())
    got, want, base = [], [], []
    for n, (o, k) in offs.items():
        if named[n].grad is None:
            continue
        want.append(named[n].grad.reshape(-1).double().cpu())
        got.append(g_fast[o:o + k].double().cpu())
        base.append(g_l1[o:o + k].double().cpu())
    got, want, base = torch.cat(got), torch.cat(want), torch.cat(base)
    err = _rel_l2(got, want)
    assert err <= tol, err
    # the term is live: the gradients differ from the L1-only ones, and in fp32 (where both routes seed the L1 part with the same
    # kernel) the difference is the autograd route's semantic contribution
    assert float((got - base).abs().max()) > 0, "the semantic term must change the gradients"
    if dt == "fp32":
        contrib = _rel_l2(got - base, want - base)
        assert contrib <= 5e-2, contrib
    assert torch.equal(per, sl.last_per_sample)


def test_add_output_grad_errors_and_batch_limit():
    from m2trans_amd import _lib
    from m2trans_amd._lib import M2TError
    model, x, hr = _model_and_inputs("fp32")
    plan = model._plan_for(x)
    lib = _lib.load()
    out = torch.empty(1, device="cuda")
    g = torch.zeros(2, 3, 224, 224, device="cuda")
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    sr = torch.empty_like(hr)
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(x), _lib.ptr(sr), 1.0, 1, ws, st), "m2t_forward")
    # no seed yet
    assert lib.m2t_add_output_grad(plan.handle, _lib.ptr(g), 224, 224, None, 1.0, 1.0, ws, st) == _lib_err("STATE")
    # a deferred L1 seed is not materialised
    _lib.check(lib.m2t_l1_loss_deferred(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(out), ws, st), "deferred")
    assert lib.m2t_add_output_grad(plan.handle, _lib.ptr(g), 224, 224, None, 1.0, 1.0, ws, st) == _lib_err("STATE")
    _lib.check(lib.m2t_l1_loss(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(out), ws, st), "l1")
    ok = (C.c_int * 4)(0, 0, 32, 32)
    assert lib.m2t_add_output_grad(plan.handle, _lib.ptr(g), 224, 224, ok, 1.0, 1.0, ws, st) == 0
    bad = (C.c_int * 4)(0, 0, 40, 33)          # 40 + 224 > 256
    assert lib.m2t_add_output_grad(plan.handle, _lib.ptr(g), 224, 224, bad, 1.0, 1.0, ws, st) == _lib_err("ARG")
    torch.cuda.synchronize()
    sl = _loss("fp32", 3, max_batch=2)
    sl.set_text_features({c: torch.ones(512) for c in "abc"})
    with pytest.raises(M2TError):
        sl.batch(torch.rand(3, 3, 256, 256, device="cuda", requires_grad=True), torch.rand(3, 3, 256, 256, device="cuda"), list("abc"))


def _lib_err(kind):
    return {"ARG": -2, "STATE": -3}[kind]


def test_full_size_bf16_train_step():
    """configs[2] geometry: x4, 128^2 LR, batch 32, 8 blocks, 32 SR crops with gradient."""
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    from tests.gpu_util import make_args
    B = 32
    model = create_model(make_args(4, 8, "bf16")).cuda()
    sl = _loss("bf16", 3, max_batch=B)
    g = torch.Generator().manual_seed(3)
    caps = [f"c{i}" for i in range(B)]
    sl.set_text_features({c: torch.randn(512, generator=g) for c in caps})
    gen = torch.Generator(device="cuda").manual_seed(9)
    lr = torch.rand(B, 3, 128, 128, generator=gen, device="cuda")
    hr = torch.rand(B, 3, 512, 512, generator=gen, device="cuda")
    ts = TrainStep(model, world_size=1, semantic_loss=sl, lambda_clip=0.01)
    torch.manual_seed(0)
    loss = ts.forward_backward(lr, hr, caps)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(ts.grads).all()
    tot, gsem, origins = sl._value_and_grad(model(lr).detach(), hr, caps)
    assert torch.isfinite(gsem).all() and float(gsem.abs().max()) > 0
    assert float(sl.last_per_sample.sum()) > 0
