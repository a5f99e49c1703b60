"""CPU tests (no GPU) of gradient accumulation: the interface of TrainStep(accum_steps=k) down to the exported symbol, and the
partition math it rests on, checked on the oracle.

A micro-batch is a rank that runs later on the same device (m2trans_amd/dist.py): every share divides its L1 sum by the element
count of the WHOLE batch -- all samples of all micro-batches of all ranks -- and the SUM of the shares' gradients is the
full-batch gradient.  Nothing couples samples (InstanceNorm per (b, c), attention per window), so the only difference between
the sum of the shares and the full batch is the order of fp32 additions."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from oracle import m2trans_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scale, n_blocks, batch, LR height, LR width: the shapes of tests/test_gpu_model.py::test_backward_fp32_every_parameter at batch 4
SHAPES = [(4, 2, 4, 32, 32), (3, 1, 4, 40, 56), (2, 1, 4, 32, 32)]


def test_interface_reaches_from_the_constructor_to_the_exported_symbol():
    from m2trans_amd import _lib
    from m2trans_amd.dist import global_divisor
    from m2trans_amd.train_step import TrainStep
    for n, w, k in ((3 * 128 * 128, 1, 1), (16 * 3 * 512 * 512, 8, 8), (7, 2, 3)):
        assert global_divisor(n, w, k) == n * w * k
        assert global_divisor(n, w) == n * w == global_divisor(n, w, 1)
        assert isinstance(global_divisor(n, w, k), float)
    par = inspect.signature(TrainStep.__init__).parameters
    assert "accum_steps" in par and par["accum_steps"].default == 1
    assert "m2t_grad_accumulate" in _lib.ABI["m2t.h"]
    res, args = _lib.ABI["m2t.h"]["m2t_grad_accumulate"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    hdr = open(os.path.join(ROOT, "include", "m2t.h")).read()
    assert re.search(r"\bint\s+m2t_grad_accumulate\s*\(\s*float\*\s*acc,\s*const float\*\s*g,\s*long long n,\s*float\*\s*loss_acc,"
                     r"\s*const float\*\s*loss_part,\s*void\*\s*stream\)", hdr)
    lib = _lib.load()
    assert hasattr(lib, "m2t_grad_accumulate")
    # the argument errors are decided on the host, before anything touches a device
    assert lib.m2t_grad_accumulate(None, None, -1, None, None, None) != 0
    assert lib.m2t_grad_accumulate(None, None, 4, None, None, None) != 0
    assert b"m2t_grad_accumulate" in lib.m2t_last_error_string()


@pytest.mark.parametrize("scale,nb,B,H0,W0", SHAPES)
def test_sum_of_micro_batch_gradients_is_the_full_batch_gradient(scale, nb, B, H0, W0):
    """2 "ranks" x 2 micro-batches of one sample each, every one with global_divisor(chunk numel, 2, 2): the sum of the four
    gradients against the oracle's full-batch gradient, every parameter tensor <= 1e-4 of its largest element (the gate of
    tests/test_gpu_model.py::test_backward_fp32_every_parameter; the fp32 oracle itself sits at ~1e-5 of an fp64 evaluation), and
    the sum of the four losses within 1e-6 of the full-batch loss."""
    from m2trans_amd.dist import global_divisor
    world, k = 2, 2
    p = O.closed_form_params(64, scale, nb)
    x = O.closed_form_image(B, 3, H0, W0)
    hr = O.closed_form_image(B, 3, H0 * scale, W0 * scale, phase=0.7)
    loss_full, _, g_full = O.l1_loss_and_grads(x, hr, p, scale, nb)
    b = B // (world * k)
    assert b * world * k == B
    loss_sum, g_sum = None, None
    for i in range(world * k):                       # rank-major, micro-batch-minor: the sample order of the full batch
        cx, chr_ = x[i * b:(i + 1) * b], hr[i * b:(i + 1) * b]
        div = global_divisor(chr_.numel(), world, k)
        assert div == hr.numel()
        li, _, gi = O.l1_loss_and_grads(cx, chr_, p, scale, nb, loss_divisor=div)
        loss_sum = li if loss_sum is None else loss_sum + li
        g_sum = gi if g_sum is None else {n: g_sum[n] + gi[n] for n in gi}
    assert abs(float(loss_sum) - float(loss_full)) < 1e-6, (float(loss_sum), float(loss_full))
    rows = [(n, float((g_sum[n] - g_full[n]).abs().max() / (g_full[n].abs().max() + 1e-30))) for n in g_full]
    print(f"x{scale} nb{nb} {H0}x{W0}: worst tensor {max(e for _, e in rows):.3e}, loss diff {abs(float(loss_sum) - float(loss_full)):.3e}")
    bad = [(n, e) for n, e in rows if not (e < 1e-4)]
    assert not bad, "\n".join(f"{n:40s} {e:.3e}" for n, e in bad)


def test_export_checkpoint_refuses_a_train_step_in_the_middle_of_a_cycle():
    """The attribute is read with a default: an object without it (accum_steps = 1 never sets it off zero) exports as before."""
    import types
    from m2trans_amd import _lib
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.checkpoint import export_checkpoint
    m = create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))
    plain = types.SimpleNamespace(lr=1e-4, step_count=0)
    assert "optimizer_state_dict" in export_checkpoint(m, plain)
    mid = types.SimpleNamespace(lr=1e-4, step_count=0, accum_steps=2, micro_count=1)
    with pytest.raises(_lib.M2TError, match="1 of 2"):
        export_checkpoint(m, mid)
    mid.micro_count = 0
    assert "optimizer_state_dict" in export_checkpoint(m, mid)


def test_timing_tool_host_part_runs_without_a_device():
    """tools/accum_timing.py: argument parsing, the shapes of configs[3]'s whole workload and the keys of the JSON line."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("accum_timing", os.path.join(ROOT, "tools", "accum_timing.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    args = T.parse_args([])
    assert (args.accum_steps, args.micro_batch, args.dtype, args.blocks) == (8, 32, "bf16", 8) and args.repeats >= 5
    assert T.shapes(args) == ((256, 3, 128, 128), (256, 3, 512, 512))
    with pytest.raises(SystemExit):
        T.parse_args(["--repeats", "4"])
    out = T.result(args, [100.0, 101.0, 99.0, 100.5, 100.0], [102.0, 101.0, 103.0, 102.0, 102.5])
    assert tuple(out) == T.RESULT_KEYS
    assert out["effective_batch"] == 256 and out["accum_patches_per_s"] == 2560.0
    assert out["plain_spread"] == round(2.0 / 102.0, 4) and out["accum_within_plain_spread"] is True
    assert T.result(args, [110.0] * 5, [100.0, 100.0, 101.0, 100.0, 100.0])["accum_within_plain_spread"] is False
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="needs a HIP device"):
            T.main([])
