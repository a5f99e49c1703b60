"""CPU tests of the input-gradient / frozen-stage backward (m2t_backward_ex) and of copying an M2Trans module:
the C ABI's argument and state checks (reached before any HIP call), the stage flags the autograd node derives from
requires_grad, and copy.deepcopy / torch.save round trips."""
import copy
import ctypes as C
import io
import os

import pytest
import torch

from tests.gpu_util import make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M2T_ERR_ARG, M2T_ERR_STATE = -2, -3


def _model(scale=4, nb=2):
    from m2trans_amd.M2Trans_network import create_model
    torch.manual_seed(0)
    return create_model(make_args(scale, nb, "fp32"))


def test_backward_ex_is_declared_exported_and_bound():
    from m2trans_amd import _lib
    assert "m2t_backward_ex" in open(os.path.join(ROOT, "include", "m2t.h")).read()
    assert "m2t_backward_ex" in _lib.ABI["m2t.h"]
    lib = _lib.load()
    assert hasattr(lib, "m2t_backward_ex")
    assert lib.m2t_backward_ex.restype is C.c_int


@pytest.mark.parametrize("nb", [1, 3])
def test_backward_ex_argument_and_state_errors(nb):
    from m2trans_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.m2t_plan_create(C.byref(h), 1, 32, 32, 4, nb, _lib.F32), "m2t_plan_create")
    try:
        buf = (C.c_float * 16)()                     # stand-in pointers: every check below runs before the first HIP call
        ptr = C.cast(buf, C.c_void_p)
        nst = nb + 2
        none = (C.c_ubyte * nst)(*([0] * nst))
        head = (C.c_ubyte * nst)(*([1] + [0] * (nst - 1)))
        tail = (C.c_ubyte * nst)(*([0] * (nst - 1) + [1]))
        call = lambda x, grads, gx, flags: lib.m2t_backward_ex(h, ptr, x, grads, gx, flags, ptr, None)
        # nothing requested
        assert call(ptr, ptr, None, none) == M2T_ERR_ARG
        assert b"nothing requested" in lib.m2t_last_error_string()
        # a stage flag without a gradient buffer (also the implicit all-stages mask)
        assert call(ptr, None, ptr, tail) == M2T_ERR_ARG
        assert b"grads is NULL" in lib.m2t_last_error_string()
        assert call(ptr, None, None, None) == M2T_ERR_ARG
        # the head's weight gradient reads x
        assert call(None, ptr, None, head) == M2T_ERR_ARG
        # null plan / params / workspace
        assert lib.m2t_backward_ex(None, ptr, ptr, ptr, ptr, None, ptr, None) == M2T_ERR_ARG
        assert lib.m2t_backward_ex(h, None, ptr, ptr, ptr, None, ptr, None) == M2T_ERR_ARG
        assert lib.m2t_backward_ex(h, ptr, ptr, ptr, ptr, None, None, None) == M2T_ERR_ARG
        # well-formed requests before any forward / seed: a state error
        for x, grads, gx, flags in ((ptr, ptr, None, None), (None, None, ptr, none), (None, ptr, ptr, tail), (ptr, ptr, ptr, head)):
            assert call(x, grads, gx, flags) == M2T_ERR_STATE
            assert b"needs m2t_forward and a seed" in lib.m2t_last_error_string()
        # m2t_backward keeps its own checks
        assert lib.m2t_backward(h, ptr, ptr, ptr, ptr, None) == M2T_ERR_STATE
        assert lib.m2t_backward(h, ptr, ptr, None, ptr, None) == M2T_ERR_ARG
    finally:
        lib.m2t_plan_destroy(h)


def test_stage_flags_follow_requires_grad():
    m = _model(4, 2)
    assert m.stage_flags() == [True, True, True, True]
    m.body.requires_grad_(False)
    assert m.stage_flags() == [True, False, False, True]
    m.requires_grad_(False)
    m.tail.requires_grad_(True)
    assert m.stage_flags() == [False, False, False, True]
    m.requires_grad_(False)
    m.head.requires_grad_(True)
    assert m.stage_flags() == [True, False, False, False]
    m.requires_grad_(False)
    assert m.stage_flags() == [False, False, False, False]
    # one tensor frozen inside a block keeps the block (and everything else) needed
    m.requires_grad_(True)
    m.body[1].attn3.rel_h.requires_grad_(False)
    assert m.stage_flags() == [True, True, True, True]
    # one tensor trainable inside an otherwise frozen model needs exactly its stage
    m.requires_grad_(False)
    m.body[1].feed_forward["0"].bias.requires_grad_(True)
    assert m.stage_flags() == [False, False, True, False]
    # the explicit form (what the autograd node passes: ctx.needs_input_grad of the parameters)
    n = len(m._names)
    assert m.stage_flags([False] * (n - 1) + [True]) == [False, False, False, True]
    assert m.stage_flags([True] + [False] * (n - 1)) == [True, False, False, False]
    # x2 / x3 tails have other names; every tail parameter maps to the last flag
    m3 = _model(3, 1)
    m3.requires_grad_(False)
    m3.tail["3"].weight.requires_grad_(True)
    assert m3.stage_flags() == [False, False, True]


def _views_of_own_flat(m):
    base = m.flat_params.data_ptr()
    return all(p.data_ptr() == base + 4 * o and p.numel() == k for (_, p), (o, k, _) in zip(m._trainable(), m._slots))


def test_deepcopy_gets_its_own_flat_buffer_and_no_plans():
    m = _model(4, 2)
    m.attach_flat_grads()
    m._plans[("fake",)] = object()                   # a plan must never be shared with a copy
    c = copy.deepcopy(m)
    assert _views_of_own_flat(c) and _views_of_own_flat(m)
    assert c.flat_params.data_ptr() != m.flat_params.data_ptr()
    assert not set(p.data_ptr() for p in c.parameters()) & set(p.data_ptr() for p in m.parameters())
    assert len(c._plans) == 0 and c._dp_pool == {} and c._dp_master is None
    assert c._dp_lock is not m._dp_lock
    assert len(m._plans) == 1
    sd_m, sd_c = m.state_dict(), c.state_dict()
    assert list(sd_m) == list(sd_c) and all(torch.equal(sd_m[k], sd_c[k]) for k in sd_m)
    # the copy is independent: writing through its parameters changes its flat buffer only
    with torch.no_grad():
        c.head.weight.add_(1.0)
    assert torch.equal(c.flat_params[:c.head.weight.numel()], c.head.weight.reshape(-1))
    assert not torch.equal(c.head.weight, m.head.weight)
    # a frozen copy (the usual teacher / fixed operator) keeps the requires_grad pattern
    m.body.requires_grad_(False)
    f = copy.deepcopy(m)
    assert f.stage_flags() == [True, False, False, True]


def test_torch_save_load_round_trips_the_module():
    m = _model(2, 1)
    m.tail.requires_grad_(False)
    f = io.BytesIO()
    torch.save(m, f)
    f.seek(0)
    r = torch.load(f, weights_only=False)
    assert type(r) is type(m) and _views_of_own_flat(r)
    assert len(r._plans) == 0
    sd_m, sd_r = m.state_dict(), r.state_dict()
    assert list(sd_m) == list(sd_r) and all(torch.equal(sd_m[k], sd_r[k]) for k in sd_m)
    assert r.stage_flags() == [True, True, False]
    assert r._slots == m._slots and r._names == m._names
