"""CPU tests (no GPU) of the inference plan: option "inference" of include/m2t.h, its forward-only workspace layout, and the Python
surface around it (Plan(inference=), M2Trans.lean_inference, train.resolve_config, the infer command line).

Host-only calls, as in tests/test_plan_surface_cpu.py: m2t_plan_create / m2t_set_option / m2t_plan_query allocate nothing on a device.
The state rules that need an initialised workspace are in tests/test_gpu_lean_inference.py.

The size bounds are derived from m2t_plan_create, not measured.  Per padded LR pixel, x4, 8 blocks:
  * training, bf16: 8 210 elements x 2 B + 384 B of fp32 (srpre, gpre) + a 1.07 GB arena; a conservative inference layout (3 X + xc + d
    + qkv + xin + a + t1act + t1der + srpre = 2.3 KB) is 0.114 of it at 512 x 512, hence the bound 0.15;
  * fp32: the plain x4 tail needs t2act: (1 056 + 1 024) x 4 B + 192 B against 33.2 KB + arena = 0.23, hence the bound 0.30.
"""
import copy
import ctypes as C
import itertools
import pickle
import types

import pytest

from tests.test_plan_surface_cpu import load_library

SMALL = (2, 40, 56)
PLANS = tuple(itertools.product((0, 1), (2, 3, 4)))      # (dtype: 0 = fp32, 1 = bf16, scale)
DEPTHS = (1, 2, 3, 8)
UNFUSED = {"fused_attn_fwd": 0, "fused_c16_fwd": 0, "fused_tail": 0}
PERSISTENT = ("zero_page", "pack_descs", "pack_blocks")   # byte-sized regions
F32_REGIONS = ("mean", "rstd", "norm_part", "srpre")       # always fp32; every other region is in the plan's element type
BACKWARD = ("gpre", "g_t2pre", "g_t1pre", "gT", "gA", "gB", "gxc", "gn", "ga", "gd", "gd2", "gdwin", "gdwin2", "head_cols", "rel_part",
            "arena", "red_descs", "col_part", "loss_part", "norm_part0") + tuple(
                f"{n}{i}{sfx}" for n in ("gqkv", "win", "relw") for i in range(4) for sfx in ("", "b"))


@pytest.fixture(scope="module")
def lib():
    from m2trans_amd import _lib
    return load_library(_lib.LIB_PATH)


class P:
    """A plan handle with its queries."""

    def __init__(self, lib, dt, scale, shape=SMALL, nb=2, inference=None, **opts):
        self.lib, self.dt, self.scale, self.nb = lib, dt, scale, nb
        self.h = C.c_void_p()
        assert lib.m2t_plan_create(C.byref(self.h), shape[0], shape[1], shape[2], scale, nb, dt) == 0
        for k, v in opts.items():
            assert self.set(k, v) == 0, k
        if inference is not None:
            assert self.set("inference", inference) == 0

    def set(self, k, v):
        return self.lib.m2t_set_option(self.h, k.encode(), v)

    def q(self, k):
        return int(self.lib.m2t_plan_query(self.h, k.encode()))

    def __del__(self):
        self.lib.m2t_plan_destroy(self.h)


def all_names(nb, scale):
    """Every workspace name a training plan of this depth knows (the inventory of tests/gpu_util.ws_float_regions + WS_PERSISTENT; the
    x4-only names are asked at every scale: absent is absent)."""
    names = ["zero_page", "pack_descs", "pack_blocks", "packed"] + [f"X{b}" for b in range(nb + 1)]
    for b in range(nb):
        names += [f"b{b}.mean", f"b{b}.rstd", f"b{b}.xc"] + [f"b{b}.{n}{i}" for i in range(1, 5) for n in ("d", "qkv")]
    return names + ["xin", "a", "norm_part", "norm_s", "vring", "t1act", "t1der", "t2act", "t2der", "srpre"] + list(BACKWARD)


def region_bytes(p, name):
    n = p.q("wsn:" + name)
    if name in PERSISTENT:
        return n
    base = name.split(".")[-1]
    return n * (4 if base in F32_REGIONS or p.dt == 0 else 2)


def test_the_option_exists_and_reads_back(lib):
    """FAILS without the feature: the key is unknown."""
    p = P(lib, 1, 4)
    assert p.q("opt:inference") == 0
    assert p.set("inference", 1) == 0
    assert p.q("opt:inference") == 1
    assert p.set("inference", 0) == 0
    assert p.q("opt:inference") == 0


@pytest.mark.parametrize("dt,scale", PLANS)
def test_setting_and_clearing_before_init_gives_an_untouched_plan(lib, dt, scale):
    keys = ["workspace_bytes", "num_params", "padded_h", "padded_w", "stores_qkv1", "stores_qkv2", "stores_t1", "stores_t2", "grad_buckets"]
    keys += [f"{f}:{n}" for n in all_names(3, scale) + ["no_such_tensor"] for f in ("ws", "wsn")]
    keys += ["opt:" + k for k in ("inference", "fused_tail", "attn_bwd", "fused_attn_fwd", "fused_c16_fwd", "fused_prep_fwd", "side_stream")]
    fresh, back = P(lib, dt, scale, nb=3), P(lib, dt, scale, nb=3)
    assert back.set("inference", 1) == 0
    assert back.q("workspace_bytes") < fresh.q("workspace_bytes")
    assert back.set("fused_tail", 0) == 0 and back.set("fused_tail", 3) == 0      # an option changed and restored in between
    assert back.set("inference", 0) == 0
    assert [back.q(k) for k in keys] == [fresh.q(k) for k in keys]
    # ... and a default plan that sees another option still sizes its workspace as before
    assert fresh.set("fused_attn_fwd", 0) == 0 and back.set("fused_attn_fwd", 0) == 0
    assert [back.q(k) for k in keys] == [fresh.q(k) for k in keys]


def expected_absent(p):
    """The regions that the schedule in force never reads in the forward, from the plan's own schedule answers."""
    bf = p.dt == 1
    fused_c16 = bf and p.q("opt:fused_c16_fwd") >= 1
    fused_c64 = bf and p.q("opt:fused_attn_fwd") >= 1
    prep_in = p.q("opt:fused_prep_fwd") == 1
    out = {"t2der"}
    if not (p.dt == 0 and p.scale == 3):      # fp32 x3: the expansion runs on the generic GEMM, whose epilogue always stores gelu' 
        out.add("t1der")
    if not (p.scale == 4 and p.q("stores_t2") == 1):
        out.add("t2act")
    if fused_c16:
        out |= {"qkv1", "d1"}
    if fused_c64:
        out |= {"qkv2", "qkv3", "qkv4"}
        if prep_in:
            out.add("d2")                      # d3 / d4 stay: the C = 256 kernel keeps its store (it spills without it)
        if p.q("opt:fused_attn_fwd2") != 0:    # the two-windows-per-CU kernels re-read the window's own v rows from the qkv tensor
            out -= {"qkv3", "qkv4"}
    return out


@pytest.mark.parametrize("opts", ({}, UNFUSED, {"fused_prep_fwd": 0}, {"fused_attn_fwd2": 1}, {"fused_attn_fwd": 1, "fused_c16_fwd": 1},
                                  {"fused_tail": 2}), ids=("default", "unfused", "prep_out", "fwd2", "stored_qkv", "tile_tail"))
@pytest.mark.parametrize("nb", DEPTHS)
@pytest.mark.parametrize("dt,scale", PLANS)
def test_layout_invariants(lib, dt, scale, nb, opts):
    p = P(lib, dt, scale, nb=nb, inference=1, **opts)
    total = p.q("workspace_bytes")
    names = all_names(nb, scale)
    present = {n: (p.q("ws:" + n), region_bytes(p, n)) for n in names if p.q("ws:" + n) >= 0}
    for n in names:
        assert (p.q("ws:" + n) < 0) == (p.q("wsn:" + n) < 0), n
    # persistent regions, X0, packed: as today
    train = P(lib, dt, scale, nb=nb, **opts)
    for n in PERSISTENT + ("packed",):
        assert (p.q("ws:" + n), p.q("wsn:" + n)) == (train.q("ws:" + n), train.q("wsn:" + n)), n
    # the X rule
    xs = [p.q(f"ws:X{b}") for b in range(nb + 1)]
    assert all(x >= 0 for x in xs)
    assert all(xs[b] != xs[b + 1] for b in range(nb)) and all(x != xs[0] for x in xs[1:])
    assert len(set(xs[1:])) == min(nb, 2)
    # ONE set of per-block regions
    for base in ("mean", "rstd", "xc") + tuple(f"{n}{i}" for i in range(1, 5) for n in ("d", "qkv")):
        answers = {(p.q(f"ws:b{b}.{base}"), p.q(f"wsn:b{b}.{base}")) for b in range(nb)}
        assert len(answers) == 1, base
    for base in ("mean", "rstd", "xc"):
        assert p.q(f"ws:b0.{base}") >= 0
    # absent regions: every backward region, and what the schedule never reads
    for n in BACKWARD:
        assert p.q("ws:" + n) == -1 and p.q("wsn:" + n) == -1, n
    absent = expected_absent(p)
    for base in ("t1der", "t2der", "t2act", "t1act"):
        if scale != 4 and base.startswith("t2"):
            assert p.q("ws:" + base) == -1
        elif base == "t1act":
            assert (p.q("ws:t1act") >= 0) == (p.q("stores_t1") == 1)
        else:
            assert (p.q("ws:" + base) == -1) == (base in absent), base
    for base in tuple(f"{n}{i}" for i in range(1, 5) for n in ("d", "qkv")):
        assert (p.q(f"ws:b0.{base}") == -1) == (base in absent), base
    for n in ("xin", "norm_part", "srpre"):
        assert n in present
    assert ("vring" in present) == (p.q("opt:fused_attn_fwd2") > 0)
    assert "a" not in present and "norm_s" not in present
    # present regions are 256-byte aligned, do not overlap, and tile [0, workspace_bytes)
    end = 0
    for off, nbytes in sorted(set(present.values())):
        assert off % 256 == 0 and nbytes > 0
        assert off == (end + 255) // 256 * 256, (off, end)
        end = off + nbytes
    assert (end + 255) // 256 * 256 == total


@pytest.mark.parametrize("dt,scale", PLANS)
def test_workspace_does_not_grow_with_depth(lib, dt, scale):
    deep, shallow = P(lib, dt, scale, nb=8, inference=1), P(lib, dt, scale, nb=2, inference=1)
    growth = 0
    for n in ("packed", "pack_descs", "pack_blocks", "b0.mean", "b0.rstd"):
        growth += region_bytes(deep, n) - region_bytes(shallow, n)
    assert deep.q("workspace_bytes") - shallow.q("workspace_bytes") <= growth + 64 * 1024


@pytest.mark.parametrize("dt,bound", ((1, 0.15), (0, 0.30)), ids=("bf16", "fp32"))
def test_size_of_one_512x512_frame(lib, dt, bound):
    shape = (1, 512, 512)
    inf, train = P(lib, dt, 4, shape, nb=8, inference=1), P(lib, dt, 4, shape, nb=8)
    ratio = inf.q("workspace_bytes") / train.q("workspace_bytes")
    print(f"dtype {dt}: inference {inf.q('workspace_bytes')} B, training {train.q('workspace_bytes')} B, ratio {ratio:.4f}")
    assert ratio <= bound


def test_state_rules_that_need_no_device(lib):
    """Without an initialised workspace the option may go back and forth and other options stay settable; an inference plan refuses a
    keeping forward and everything that needs activations before it looks at a device (null pointers would be M2T_ERR_ARG first, so the
    calls pass a non-null dummy that is never dereferenced: the refusal precedes any launch)."""
    p = P(lib, 1, 4, inference=1)
    assert p.set("fused_tail", 0) == 0 and p.q("opt:fused_tail") == 0 and p.q("ws:t2act") >= 0
    assert p.set("fused_tail", 3) == 0 and p.q("ws:t2act") == -1
    dummy = (C.c_float * 4)()
    ptr = C.cast(dummy, C.c_void_p)
    err = lambda: lib.m2t_last_error_string().decode()
    ERR_STATE = -3
    assert lib.m2t_forward(p.h, ptr, ptr, ptr, 1.0, 1, ptr, None) == ERR_STATE and "inference plan" in err()
    assert lib.m2t_l1_loss(p.h, ptr, 1.0, 1.0, 1.0, ptr, ptr, None) == ERR_STATE and "inference plan" in err()
    assert lib.m2t_l1_loss_deferred(p.h, ptr, 1.0, 1.0, 1.0, ptr, ptr, None) == ERR_STATE and "inference plan" in err()
    assert lib.m2t_set_output_grad(p.h, ptr, 1.0, ptr, None) == ERR_STATE and "inference plan" in err()
    assert lib.m2t_backward(p.h, ptr, ptr, ptr, ptr, None) == ERR_STATE and "inference plan" in err()
    assert lib.m2t_backward_ex(p.h, ptr, ptr, ptr, None, None, ptr, None) == ERR_STATE and "inference plan" in err()
    assert lib.m2t_stream_wait_bucket(p.h, 0, None) == ERR_STATE and "inference plan" in err()


def _model(**extra):
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=2, rgb_range=1.0, n_blocks=1, colors=3, compute_dtype="bf16", **extra))


def test_lean_inference_flag_is_a_plain_attribute():
    m = _model()
    assert m.lean_inference_enabled is False
    assert m.lean_inference() is m and m.lean_inference_enabled is True
    assert copy.deepcopy(m).lean_inference_enabled is True
    assert pickle.loads(pickle.dumps(m)).lean_inference_enabled is True
    assert m.lean_inference(False) is m and m.lean_inference_enabled is False
    assert copy.deepcopy(m).lean_inference_enabled is False
    assert _model(lean_inference=True).lean_inference_enabled is True
    # the replica nn.DataParallel makes is a shallow copy of the module's __dict__: the flag rides along
    m.lean_inference()
    assert m.__dict__["lean_inference_enabled"] is True


def test_inference_plans_have_their_own_cache_key(monkeypatch):
    from m2trans_amd import M2Trans_network as N
    made = []

    class FakePlan:
        def __init__(self, B, H0, W0, scale, n_blocks, dtype, device, inference=False):
            self.inference = inference
            made.append(inference)

    monkeypatch.setattr(N, "Plan", FakePlan)
    monkeypatch.setattr(N.M2Trans, "_check_plan", lambda self, plan: None)
    monkeypatch.setattr(N.M2Trans, "_device_ok", lambda self, x: None)
    m = _model()

    class X:
        shape, is_cuda = (1, 3, 32, 32), True
        device = m.flat_params.device

        def dim(self):
            return 4

    a, b = m._plan_for(X()), m._plan_for(X(), inference=True)
    assert a is not b and made == [False, True] and (a.inference, b.inference) == (False, True)
    assert m._plan_for(X()) is a and m._plan_for(X(), inference=True) is b and len(m._plans) == 2
    assert [k[-1] == "inference" for k in m._plans] == [False, True]
    with pytest.raises(N.M2TError, match="inference plan"):
        m._run_forward(b, None, keep=True)


def test_train_config_takes_lean_inference():
    from m2trans_amd import train as T
    from m2trans_amd._lib import M2TError
    cfg = {"scale": 2, "patch_size": 64, "batch_size": 4, "epochs": 1, "lr": 1e-4, "eta_min": 1e-6, "log_every": 1, "test_every": 1,
           "data_path": "/nowhere", "lambda_clip": 0}
    assert "lean_inference" in T.MODEL_KEYS and "lean_inference" in T.REFERENCE_KEYS
    assert "lean_inference" not in T.resolve_config(cfg)["model"]
    r = T.resolve_config(dict(cfg, lean_inference=True))
    assert r["model"]["lean_inference"] is True and "lean_inference" not in r["train_step"] and "lean_inference" not in r["fit"]
    assert T.resolve_config(dict(cfg, lean_inference=False))["model"]["lean_inference"] is False
    with pytest.raises(M2TError, match="lean_inference"):
        T.resolve_config(dict(cfg, lean_inference="yes"))
    from m2trans_amd.infer import model_namespace
    from m2trans_amd.M2Trans_network import create_model
    assert create_model(model_namespace(dict(r["model"], n_blocks=1))).lean_inference_enabled is True


def test_timing_tool_host_part_runs_without_a_device():
    """tools/lean_inference_timing.py: argument parsing, the four shapes and the keys of the JSON line."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("lean_inference_timing", os.path.join(root, "tools", "lean_inference_timing.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args([])
    assert (a.reps, a.repeats, a.n_blocks) == (10, 5, 8)
    assert tool.parse_args(["--reps", "3", "--repeats", "2", "--n-blocks", "1"]).n_blocks == 1
    with pytest.raises(SystemExit):
        tool.parse_args(["--reps", "0"])
    assert tool.SHAPES == (("bf16", 16, 128, 128), ("bf16", 1, 512, 512), ("bf16", 8, 256, 256), ("fp32", 16, 128, 128))
    assert tool.RESULT_KEYS == ("workload", "reps", "repeats", "n_blocks", "shapes")


def test_infer_cli_parses_lean():
    from m2trans_amd import infer
    base = ["--config", "c.yml", "--model_path", "m.pt", "--input", "in", "--output", "out"]
    assert infer.parse_args(base).lean is False
    assert infer.parse_args(base + ["--lean"]).lean is True
    assert infer.parse_args(base + ["--lean", "--self_ensemble", "--tile", "64"]).lean is True
    import inspect
    assert inspect.signature(infer.upscale_folder).parameters["lean"].default is False
