"""TransBlock backward on the device (include/m2t_rlutrans.h through m2trans_amd.rlutrans.TransBlock) against fp64 autograd of
oracle.rlutrans_oracle.trans_block: the fp32 gate, the teacher-forced bf16 gate, bit-identity of y with the inference route,
reproducibility, the null-output routes, graph reuse and a short SGD loop.  Inputs: RO.closed_form_params(), x / gy from a
generator seeded by N (tests/rlutrans_ref.inputs).  (3, 300) is the shape whose 900 rows leave more than one weight-gradient slab;
(1, 1050) is added to the issue's five because the attention backward stages its chunk in LDS from N = 512 on (tests/rlutrans_ref.STAGED)."""
import ctypes as C

import pytest
import torch

from oracle import rlutrans_oracle as RO
from tests import rlutrans_ref as RR

pytestmark = pytest.mark.gpu
P = RO.closed_form_params()
BF16_SHAPES = RR.SHAPES[2:] + (RR.STAGED,)
_CACHE = {}


def _oracle(shape):
    """fp64 autograd of the oracle, computed once per shape and shared."""
    if shape not in _CACHE:
        x, gy = RR.inputs(*shape)
        _CACHE[shape] = (x, gy) + RR.oracle_grads(x, P, gy)
    return _CACHE[shape]


def _block(dtype="fp32", params=P):
    from m2trans_amd.rlutrans import TransBlock
    m = TransBlock(compute_dtype=dtype)
    m.load_state_dict(params)
    return m.cuda()


def _run(m, x, gy, x_grad=True):
    """(y, gx, {name: grad}, autograd node) of one forward + backward through the module, everything on the host."""
    for p in m.parameters():
        p.grad = None
    xd = x.cuda().requires_grad_(x_grad)
    y = m(xd)
    node = y.grad_fn
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.cpu()) for n, p in m.named_parameters()}
    return y.detach().cpu(), (xd.grad.cpu() if x_grad else None), grads, node


def _raw(code, x, gy, fill=None, want_x=True, want_p=True):
    """The C entry points themselves on a workspace of the test's own: (y, gx, gparams)."""
    from m2trans_amd import _lib
    lib = _lib.load()
    B, N, _ = x.shape
    flat = torch.cat([P[n].reshape(-1).float() for n in RR.NAMES]).cuda()
    ws = torch.empty(int(lib.m2t_transblock_train_workspace_bytes(B, N, code)), dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    xc, gyc = x.cuda().contiguous(), gy.cuda().contiguous()
    y = torch.empty_like(xc)
    gx = torch.full_like(xc, float("nan")) if want_x else None
    gp = torch.full((_lib.TRANSBLOCK_NPARAMS,), float("nan"), device="cuda") if want_p else None
    _lib.check(lib.m2t_transblock_forward_train(_lib.ptr(flat), _lib.ptr(xc), _lib.ptr(y), B, N, code, _lib.ptr(ws), _lib.stream_ptr()))
    _lib.check(lib.m2t_transblock_backward(_lib.ptr(flat), _lib.ptr(gyc), _lib.ptr(gx), _lib.ptr(gp), B, N, code, _lib.ptr(ws),
                                           _lib.stream_ptr()))
    torch.cuda.synchronize()
    return y.cpu(), None if gx is None else gx.cpu(), None if gp is None else gp.cpu()


def _device_h1(node, B, N, code):
    from m2trans_amd import _lib
    off = int(_lib.load().m2t_transblock_train_workspace_offset(B, N, code, _lib.TRANSBLOCK_REGIONS["H1"]))
    assert off != C.c_size_t(-1).value
    es, dt = (4, torch.float32) if code == _lib.F32 else (2, torch.bfloat16)
    return node.ws[off:off + B * N * 16 * es].view(dt).reshape(B, N, 16).float().cpu()


# ---- 7
@pytest.mark.parametrize("shape", RR.SHAPES + (RR.STAGED,))
def test_fp32_gradients_against_fp64_autograd(shape):
    """rel <= 1e-4 per tensor: the project's gate for fp32 gradients against an fp64 evaluation.  At L = 1 the exact-zero q / k rows of
    atten.qkv.weight.grad are judged by the same tensor-wide bound."""
    x, gy, y, gx, grads, mask = _oracle(shape)
    yd, gxd, gd, node = _run(_block("fp32"), x, gy)
    assert float(((_device_h1(node, *shape, 0) > 0) != mask).double().mean()) <= 1e-3        # (a unit within fp32 rounding of 0 may differ)
    print(f"{shape} fp32: y {RR.rel(yd, y):.2e} gx {RR.rel(gxd, gx):.2e} " + " ".join(f"{n} {RR.rel(gd[n], grads[n]):.2e}" for n in RR.NAMES))
    assert RR.rel(yd, y) < 2e-5 and RR.rel(gxd, gx) <= 1e-4
    for n in RR.NAMES:
        assert gd[n].shape == grads[n].shape and RR.rel(gd[n], grads[n]) <= 1e-4, (n, RR.rel(gd[n], grads[n]))


# ---- 8
@pytest.mark.parametrize("shape", BF16_SHAPES)
def test_bf16_gradients_teacher_forced_within_three_times_the_emulation(shape):
    """The rule of tests/attn_ref.py per tensor: the device is no further from fp64 than 3x the CPU emulation with the kernels' own bf16
    rounding points (tests/rlutrans_ref.py, bf16=True) on the same inputs.  Both sides are teacher-forced: the fp64 reference of the
    device run takes the DEVICE's ReLU mask (read from the H1 region of the workspace), the reference of the emulation takes the
    emulation's, so a unit that rounding pushed across 0 does not count as a gradient error; the mask itself is checked first."""
    x, gy, y, gx, grads, mask = _oracle(shape)
    yd, gxd, gd, node = _run(_block("bf16"), x, gy)
    dmask = _device_h1(node, *shape, 1) > 0
    flipped = float((dmask != mask).double().mean())
    print(f"{shape} bf16: device mask differs from fp64 in {100 * flipped:.3f} %")
    assert flipped <= 0.01
    _, gx_r, g_r, _ = RR.value_and_grads(x, P, gy, mask=dmask)
    _, gx_e, g_e, emask = RR.value_and_grads(x, P, gy, bf16=True)
    _, gx_er, g_er, _ = RR.value_and_grads(x, P, gy, mask=emask)
    rows = [("gx", RR.rel(gx_e, gx_er), RR.rel(gxd, gx_r))] + [(n, RR.rel(g_e[n], g_er[n]), RR.rel(gd[n], g_r[n])) for n in RR.NAMES]
    for n, budget, err in rows:
        print(f"  {n:22s} emulation {budget:.3e}   device {err:.3e}   ratio {err / budget:.2f}")
    for n, budget, err in rows:
        assert err <= 3 * budget, (n, err, budget)


# ---- 9
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_y_of_the_training_route_is_bit_identical_to_inference(dtype):
    m = _block(dtype)
    for shape in ((2, 17), (3, 300)):
        x = RR.inputs(*shape)[0].cuda()
        with torch.no_grad():
            want = m(x)
        got = m(x)
        assert want.grad_fn is None and got.grad_fn is not None and torch.equal(got, want), shape


# ---- 10
@pytest.mark.parametrize("code", [0, 1])
def test_reproducible_and_independent_of_the_workspace_contents(code):
    for shape in ((3, 300), RR.STAGED):
        _check_reproducible(code, shape)


def _check_reproducible(code, shape):
    x, gy = RR.inputs(*shape)
    a = _raw(code, x, gy)
    b = _raw(code, x, gy)
    c = _raw(code, x, gy, fill=0xFF)
    for t in a:
        assert torch.isfinite(t).all()                      # the NaN prefill of gx / gparams is gone
    for other in (b, c):
        assert all(torch.equal(s, t) for s, t in zip(a, other))


# ---- 11
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_null_outputs_skip_work_without_changing_the_rest(dtype):
    x, gy = RR.inputs(2, 100)
    m = _block(dtype)
    _, gx_full, g_full, _ = _run(m, x, gy)
    _, none, g_only, _ = _run(m, x, gy, x_grad=False)
    assert none is None and all(torch.equal(g_only[n], g_full[n]) for n in RR.NAMES)
    for p in m.parameters():
        p.requires_grad_(False)
    _, gx_only, g_none, _ = _run(m, x, gy)
    assert torch.equal(gx_only, gx_full) and all(g is None for g in g_none.values())
    code = 0 if dtype == "fp32" else 1
    _, gx_raw, gp_raw = _raw(code, x, gy)
    assert torch.equal(gx_raw, gx_full) and torch.equal(gp_raw, torch.cat([g_full[n].reshape(-1) for n in RR.NAMES]))
    assert torch.equal(_raw(code, x, gy, want_p=False)[1], gx_full)
    assert torch.equal(_raw(code, x, gy, want_x=False)[2], gp_raw)


# ---- 12
def test_backward_twice_on_one_graph():
    x, gy = RR.inputs(2, 33)
    for dtype in ("fp32", "bf16"):
        m = _block(dtype)
        xd = x.cuda().requires_grad_(True)
        y = m(xd)
        first = torch.autograd.grad(y, [xd] + list(m.parameters()), gy.cuda(), retain_graph=True)
        second = torch.autograd.grad(y, [xd] + list(m.parameters()), gy.cuda())
        assert all(torch.equal(s, t) for s, t in zip(first, second)), dtype


def test_block_applied_twice_with_shared_weights():
    x, gy = RR.inputs(2, 33)
    m = _block("fp32")
    xd = x.cuda().requires_grad_(True)
    m(m(xd)).backward(gy.cuda())
    p = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
    xr = x.double().clone().requires_grad_(True)
    RO.trans_block(RO.trans_block(xr, p), p).backward(gy.double())
    assert RR.rel(xd.grad.cpu(), xr.grad) <= 1e-4
    for n, q in m.named_parameters():
        assert RR.rel(q.grad.cpu(), p[n].grad) <= 1e-4, (n, RR.rel(q.grad.cpu(), p[n].grad))


# ---- 13
def test_three_sgd_steps_on_a_two_block_stack_track_the_oracle():
    """loss = mean((y - target)^2) with target = gy of the shared inputs; lr = 0.1, three steps, fp32 compute."""
    x, target = RR.inputs(2, 33)
    second = {k: v.flip(-1).contiguous() for k, v in P.items()}       # a second, different parameter set
    blocks = torch.nn.Sequential(_block("fp32"), _block("fp32", second))
    opt = torch.optim.SGD(blocks.parameters(), lr=0.1)
    ref = [{k: v.double().clone().requires_grad_(True) for k, v in q.items()} for q in (P, second)]
    ropt = torch.optim.SGD([t for q in ref for t in q.values()], lr=0.1)
    for _ in range(3):
        opt.zero_grad()
        ((blocks(x.cuda()) - target.cuda()) ** 2).mean().backward()
        opt.step()
        ropt.zero_grad()
        ((RO.trans_block(RO.trans_block(x.double(), ref[0]), ref[1]) - target.double()) ** 2).mean().backward()
        ropt.step()
    for blk, q, start in zip(blocks, ref, (P, second)):
        for n, t in blk.named_parameters():
            assert RR.rel(t.detach().cpu(), q[n].detach()) <= 1e-4, (n, RR.rel(t.detach().cpu(), q[n].detach()))
            assert not torch.equal(q[n].detach().float(), start[n]), n            # the step moved it


# ---- 14
def test_training_route_raises_like_the_inference_route():
    from m2trans_amd._lib import M2TError
    m = _block("fp32")
    assert torch.is_grad_enabled() and all(p.requires_grad for p in m.parameters())
    with pytest.raises(M2TError):
        m(torch.zeros(2, 15, 64, device="cuda", requires_grad=True))
    with pytest.raises(M2TError):
        m(torch.zeros(2, 32, 64, requires_grad=True))
    from m2trans_amd import _lib
    lib = _lib.load()
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(M2TError, match="N >= 16"):
        _lib.check(lib.m2t_transblock_forward_train(_lib.ptr(ws), _lib.ptr(ws), _lib.ptr(ws), 2, 15, 0, _lib.ptr(ws), _lib.stream_ptr()))
