"""TransBlock backward without a device: the fp64 restatement of the eight backward steps (tests/rlutrans_ref.py) against fp64
autograd of the oracle, the C ABI table of include/m2t_rlutrans.h, the argument handling of its four entry points, the routing of
``TransBlock.forward`` against a recording stand-in for the library, the ReLU-mask condition the bf16 GPU gate relies on, and the
host part of tools/transblock_timing.py."""
import contextlib
import ctypes as C
import os
import re

import pytest
import torch

from oracle import rlutrans_oracle as RO
from tests import rlutrans_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = RO.closed_form_params()


@pytest.fixture(scope="module")
def oracle():
    """fp64 autograd of the oracle, once per shape."""
    out = {}
    for B, N in RR.SHAPES + (RR.STAGED,):
        x, gy = RR.inputs(B, N)
        out[(B, N)] = (x, gy) + RR.oracle_grads(x, P, gy)
    return out


def test_inputs_reach_every_parameter_and_about_half_the_hidden_units(oracle):
    for shape, (x, gy, y, gx, grads, mask) in oracle.items():
        assert all(float(g.abs().max()) > 0 for g in grads.values()), shape
        assert 0.35 < float(mask.double().mean()) < 0.65, (shape, float(mask.double().mean()))
    # L = 1: softmax over one key, so q and k receive exactly nothing
    for shape in ((2, 16), (2, 17)):
        g = oracle[shape][4]["atten.qkv.weight"]
        assert int(torch.count_nonzero(g[:128])) == 0 and float(g[128:].abs().max()) > 0


@pytest.mark.parametrize("shape", RR.SHAPES[:4])
def test_restated_backward_equals_autograd_of_the_oracle(oracle, shape):
    x, gy, y, gx, grads, mask = oracle[shape]
    y2, gx2, g2, m2 = RR.value_and_grads(x, P, gy)
    assert torch.equal(m2, mask)
    assert RR.rel(y2, y) <= 1e-10 and RR.rel(gx2, gx) <= 1e-10
    for n in RR.NAMES:
        assert g2[n].shape == grads[n].shape and RR.rel(g2[n], grads[n]) <= 1e-10, (n, RR.rel(g2[n], grads[n]))
    if shape[1] < 32:       # L = 1: delta is taken from the stored AO as the kernels do, so the q and k rows are rounding dust, not 0
        assert float(g2["atten.qkv.weight"][:128].abs().max()) <= 1e-12 * float(g2["atten.qkv.weight"].abs().max())


@pytest.mark.parametrize("shape", RR.SHAPES[:4])
def test_forcing_the_own_mask_changes_no_bit(shape):
    x, gy = RR.inputs(*shape)
    for bf16 in (False, True):
        y, gx, g, m = RR.value_and_grads(x, P, gy, bf16=bf16)
        y2, gx2, g2, m2 = RR.value_and_grads(x, P, gy, mask=m, bf16=bf16)
        assert torch.equal(y, y2) and torch.equal(gx, gx2) and torch.equal(m, m2)
        assert all(torch.equal(g[n], g2[n]) for n in RR.NAMES)


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_refuse_bad_arguments_before_any_launch():
    from m2trans_amd import _lib
    lib = _lib.load()
    bad_off = C.c_size_t(-1).value
    for dt in (_lib.F32, _lib.BF16):
        assert lib.m2t_transblock_train_workspace_bytes(0, 16, dt) == 0 and lib.m2t_transblock_train_workspace_bytes(2, 15, dt) == 0
        total = lib.m2t_transblock_train_workspace_bytes(2, 33, dt)
        offs = [lib.m2t_transblock_train_workspace_offset(2, 33, dt, r) for r in _lib.TRANSBLOCK_REGIONS.values()]
        assert total > 0 and len(set(offs)) == len(offs) and all(o % 256 == 0 and o < total for o in offs)
        assert lib.m2t_transblock_train_workspace_offset(2, 33, dt, len(offs)) == bad_off
        assert lib.m2t_transblock_train_workspace_offset(2, 33, dt, -1) == bad_off
        assert lib.m2t_transblock_train_workspace_offset(2, 15, dt, 0) == bad_off
    assert lib.m2t_transblock_train_workspace_bytes(2, 33, 7) == 0
    assert lib.m2t_transblock_train_workspace_bytes(2, 33, _lib.F32) > lib.m2t_transblock_train_workspace_bytes(2, 33, _lib.BF16)
    one = C.c_void_p(8)                                              # a non-null pointer that is never followed
    fwd = lambda **kw: lib.m2t_transblock_forward_train(*[kw.get(k, v) for k, v in (
        ("params", one), ("x", one), ("y", one), ("B", 2), ("N", 33), ("dt", 0), ("ws", one), ("stream", None))])
    bwd = lambda **kw: lib.m2t_transblock_backward(*[kw.get(k, v) for k, v in (
        ("params", one), ("gy", one), ("gx", one), ("gp", one), ("B", 2), ("N", 33), ("dt", 0), ("ws", one), ("stream", None))])
    for bad in (dict(params=None), dict(x=None), dict(y=None), dict(ws=None), dict(N=15), dict(B=0), dict(dt=2)):
        assert fwd(**bad) == -2, bad
        assert lib.m2t_last_error_string().decode().startswith("m2t_transblock_forward_train")
    for bad in (dict(params=None), dict(gy=None), dict(ws=None), dict(gx=None, gp=None), dict(N=15), dict(B=0), dict(dt=-1)):
        assert bwd(**bad) == -2, bad
        assert lib.m2t_last_error_string().decode().startswith("m2t_transblock_backward")


# ------------------------------------------------------------------------------------------------------------- routing
class _Calls:
    """A stand-in for the loaded library: records (entry point, arguments) in call order, every call succeeds."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def fn(*a):
            self.log.append((name, a))
            return 4096 if name.endswith("_bytes") else 0
        return fn

    @property
    def names(self):
        return [n for n, _ in self.log]


@pytest.fixture
def host(monkeypatch):
    from m2trans_amd import _lib, rlutrans
    calls = _Calls()
    monkeypatch.setattr(_lib, "load", lambda: calls)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(_lib, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(rlutrans, "_require_device", lambda x: None)
    m = rlutrans.TransBlock()
    m.load_state_dict(P)
    return calls, m


INFER = ["m2t_transblock_workspace_bytes", "m2t_transblock_forward"]
TRAIN = ["m2t_transblock_train_workspace_bytes", "m2t_transblock_forward_train"]


def test_routing_inference_issues_the_two_calls_it_always_did(host):
    calls, m = host
    x = torch.zeros(2, 33, 64)
    with torch.no_grad():
        y = m(x)
    assert calls.names == INFER and y.grad_fn is None
    calls.log.clear()
    with torch.no_grad():
        m(x.clone().requires_grad_(True))                        # requires_grad under no_grad: still inference
    assert calls.names == INFER
    calls.log.clear()
    for p in m.parameters():
        p.requires_grad_(False)
    y = m(x)                                                     # grad mode on, nothing requires grad
    assert calls.names == INFER and y.grad_fn is None


def test_routing_training_and_null_outputs(host):
    calls, m = host
    x = torch.zeros(2, 33, 64)
    y = m(x)
    assert calls.names == TRAIN and y.grad_fn is not None
    y.sum().backward()
    assert calls.names == TRAIN + ["m2t_transblock_backward"]
    name, a = calls.log[-1]
    assert a[2] is None and a[3] is not None and a[4:7] == (2, 33, 0)          # x needs no gradient: gx is null
    assert a[0] == calls.log[1][1][0] and a[7] == calls.log[1][1][6]           # the forward's own flat vector and workspace
    grads = [p.grad for p in m.parameters()]
    assert [tuple(g.shape) for g in grads] == [tuple(p.shape) for p in m.parameters()]
    base = grads[0].untyped_storage().data_ptr()
    assert all(g.untyped_storage().data_ptr() == base for g in grads)           # 12 views of one buffer
    # every parameter frozen, x requires grad: gparams is null and no parameter receives a gradient
    calls.log.clear()
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
    xg = x.clone().requires_grad_(True)
    m(xg).sum().backward()
    name, a = calls.log[-1]
    assert calls.names == TRAIN + ["m2t_transblock_backward"] and a[2] is not None and a[3] is None
    assert xg.grad is not None and all(p.grad is None for p in m.parameters())
    # one parameter frozen: it gets None, the others their views
    calls.log.clear()
    for p in m.parameters():
        p.requires_grad_(True)
    m.norm1.weight.requires_grad_(False)
    m(x).sum().backward()
    assert m.norm1.weight.grad is None and m.norm1.bias.grad is not None and calls.log[-1][1][3] is not None


def test_routing_two_forwards_hold_two_workspaces(host):
    calls, m = host
    x = torch.zeros(2, 33, 64)
    y1, y2 = m(x), m(x)
    (y1.sum() + y2.sum()).backward()
    assert calls.names == TRAIN + TRAIN + ["m2t_transblock_backward"] * 2
    f1, f2 = calls.log[1][1], calls.log[3][1]
    assert f1[6] != f2[6] and f1[0] != f2[0]                                     # workspaces and flat vectors of their own
    b = sorted((a[7], a[0]) for n, a in calls.log[4:])
    assert b == sorted([(f1[6], f1[0]), (f2[6], f2[0])])                         # each backward on its forward's pair


def test_bf16_code_reaches_both_calls(host):
    calls, m = host
    m.compute_dtype = "bf16"
    m(torch.zeros(1, 16, 64)).sum().backward()
    assert calls.log[1][1][3:6] == (1, 16, 1) and calls.log[2][1][4:7] == (1, 16, 1)


# ------------------------------------------------------------------------------------------------------------- bf16 mask condition
@pytest.mark.parametrize("shape", RR.SHAPES + (RR.STAGED,))
def test_bf16_forward_emulation_keeps_the_relu_mask(oracle, shape):
    """The bf16 GPU gate is teacher-forced with the device's own mask; that is only meaningful while rounding flips few units."""
    x, gy, y, gx, grads, mask = oracle[shape]
    yb, _, _, mb = RR.value_and_grads(x, P, gy, bf16=True)
    flipped = float((mb != mask).double().mean())
    print(f"{shape}: bf16 emulation flips {100 * flipped:.3f} % of the ReLU mask; y rel {RR.rel(yb, y):.2e}")
    assert flipped <= 0.01
    assert RR.rel(yb, y) < 3e-2                                  # the forward's own bf16 tolerance (tests/test_rlutrans.py)
    # the emulation really rounds: every stored tensor it returns is a bf16 value
    assert torch.equal(yb, yb.to(torch.bfloat16).double())


# ------------------------------------------------------------------------------------------------------------- timing tool
def test_timing_tool_host_part_runs_without_a_device():
    """tools/transblock_timing.py: argument parsing, the keys of the JSON line, and its eager block against the oracle."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("transblock_timing", os.path.join(ROOT, "tools", "transblock_timing.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    args = T.parse_args([])
    assert (args.batch, args.tokens, args.dtypes) == (16, [2304, 4096], ["fp32", "bf16"]) and args.repeats >= 3
    for bad in (["--repeats", "2"], ["--tokens", "15"], ["--calls", "0"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
    ms = {"infer": [1.0, 1.1, 0.9], "fwd_train": [1.0, 1.0, 1.0], "bwd": [2.0, 2.0, 2.2], "bwd_data": [1.5, 1.5, 1.5], "eager": [9.0, 9.0, 9.0]}
    out = T.case_result(4096, "bf16", ms, 3 << 20, 1.5e-6)
    assert tuple(out) == T.CASE_KEYS and out["train_ms"] == 3.0 and out["eager_over_train"] == 3.0 and out["workspace_mib"] == 3.0
    assert out["spread"]["infer"] == 0.2 and out["spread"]["bwd"] == 0.1
    # the eager yardstick computes the block: the batched form (16 | N) and the chunk loop (a 17th, shorter chunk)
    for B, N in ((2, 32), (2, 33)):
        x = RR.inputs(B, N)[0].double()
        p = {k: v.double() for k, v in P.items()}
        assert RR.rel(T.eager_block(x, p), RO.trans_block(x, p)) <= 1e-12
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="needs a HIP device"):
            T.main([])
