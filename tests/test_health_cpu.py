"""CPU tests (no GPU) of the step health record: option "health" of include/m2t.h, its rows and queries on plans built on the host
(as tests/test_lean_plan_cpu.py does), the restatement tests/health_ref.py, the fp8 arithmetic of m2trans_amd/health.py, the
``track_health`` config key and log line, and the device text of csrc/m2t_health_tile.h run on the host by the stand-alone program
tests/health_emulate.cpp (built with -fsanitize=address,undefined, run as a program) over adversarial buffers.

Every test fails on a library without the option: m2t_set_option(plan, "health", ...) is an unknown key there.
The rules that need an initialised workspace, and every device figure, are in tests/test_gpu_health.py.
"""
import os
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest

from tests import health_ref as R
from tests.test_lean_plan_cpu import P, PLANS, UNFUSED, all_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_KEYS = ("side_stream", "fork_on_kernel", "fp32_fast", "tail_bwd_mfma32", "fused_l1", "fused_attn_fwd2", "fused_norm_red", "fused_prep_fwd",
            "fused_prep_bwd", "gate_branch", "wgrad_big_tiles", "fused_tail", "attn_bwd", "conv_rows", "fused_conv_bwd", "fused_attn_fwd",
            "fused_c16_fwd", "inference", "local_norm")


@pytest.fixture(scope="module")
def lib():
    from m2trans_amd import _lib
    from tests.test_plan_surface_cpu import load_library
    return load_library(_lib.LIB_PATH)


def _err(lib):
    return lib.m2t_last_error_string().decode()


def _names(lib, p):
    out = []
    for i in range(p.q("health_rows")):
        n = p.q(f"health_name:{i}")
        name = _err(lib)
        assert n == len(name) and p.q("health_row:" + name) == i
        out.append(name)
    return out


def _expected(p, level):
    """The rows, restated from the issue: sr; every region the forward writes whose ws: offset is >= 0 and which the options in force
    store; at level 2 the regions the backward leaves; grads."""
    nb, x4 = p.nb, p.scale == 4
    fwd = ["sr", "X0"]
    for b in range(nb):
        fwd += [f"b{b}.mean", f"b{b}.rstd"]
        for i in range(1, 5):
            fwd.append(f"b{b}.d{i}")
            if i >= 3 or p.q(f"stores_qkv{i}"):
                fwd.append(f"b{b}.qkv{i}")
        fwd += [f"b{b}.xc", f"X{b + 1}"]
    if p.q("stores_t1"):
        fwd += ["t1act", "t1der"]
    if p.q("stores_t2"):
        fwd += ["t2act", "t2der"]
    fwd.append("srpre")
    fwd = [n for n in fwd if n == "sr" or p.q("ws:" + n) >= 0]
    bwd = []
    if level >= 2:
        plain_tail = p.q("opt:fused_tail") == 0
        bwd += ["g_t2pre"] if x4 and plain_tail else []
        bwd += ["g_t1pre"] if x4 or plain_tail else []
        bwd += ["gT"] + (["gA"] if nb >= 3 else []) + (["gB"] if nb >= 2 else [])
        bwd += [f"gqkv{i}" for i in range(4)] + ([f"gqkv{i}b" for i in range(4)] if nb >= 2 else [])
        bwd += ["gn", "gxc"]
        assert all(p.q("ws:" + n) >= 0 for n in bwd)
        bwd.append("grads")
    return fwd, bwd


# ------------------------------------------------------------------------------------------------------------- the option
@pytest.mark.parametrize("dt,scale", PLANS)
def test_level_0_is_a_plan_that_never_heard_of_the_option(lib, dt, scale):
    fresh, off, back = P(lib, dt, scale), P(lib, dt, scale, health=0), P(lib, dt, scale, health=2)
    assert back.q("workspace_bytes") > fresh.q("workspace_bytes") and back.q("ws:health") > 0
    assert back.set("health", 0) == 0
    keys = ["workspace_bytes", "num_params", "padded_h", "padded_w", "stores_qkv1", "stores_qkv2", "stores_t1", "stores_t2", "health_rows",
            "ws:health", "ws:health_part", "wsn:health", "health_row:sr", "health_row:X0", "health_phase:0", "health_name:0", "opt:health",
            "opt:health_on"]
    keys += [f"{f}:{n}" for n in all_names(2, scale) for f in ("ws", "wsn")] + ["opt:" + k for k in OPT_KEYS]
    for k in keys:
        assert fresh.q(k) == off.q(k) == back.q(k), k
    assert fresh.q("ws:health") == -1 and fresh.q("health_rows") == 0 and fresh.q("opt:health") == 0
    assert fresh.set("health_on", 0) == 0 and fresh.set("health_on", 1) == 0            # accepted, no effect
    assert fresh.q("workspace_bytes") == off.q("workspace_bytes")


@pytest.mark.parametrize("opts", ({}, UNFUSED), ids=("default", "unfused"))
@pytest.mark.parametrize("nb", (1, 2, 3))
@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("dt,scale", PLANS)
def test_rows_are_the_stored_tensors_in_pass_order(lib, dt, scale, level, nb, opts):
    p = P(lib, dt, scale, nb=nb, health=level, **opts)
    plain = P(lib, dt, scale, nb=nb, **opts)
    fwd, bwd = _expected(p, level)
    names = _names(lib, p)
    assert names == fwd + bwd
    assert p.q("opt:health") == level and p.q("opt:health_on") == 1
    phases = [p.q(f"health_phase:{i}") for i in range(len(names))]
    assert phases == [0] * len(fwd) + [1] * len(bwd)                                    # forward rows precede backward rows
    assert p.q(f"health_phase:{len(names)}") == -1 and p.q(f"health_name:{len(names)}") == -1 and p.q("health_phase:x") == -1
    # no row for a tensor the options in force do not store, nor for a scratch region
    for n in ("b0.qkv1", "b0.qkv2", "t1act", "t1der", "t2act", "t2der"):
        stored = {"b0.qkv1": "stores_qkv1", "b0.qkv2": "stores_qkv2", "t1act": "stores_t1", "t1der": "stores_t1", "t2act": "stores_t2",
                  "t2der": "stores_t2"}[n]
        assert (p.q("health_row:" + n) >= 0) == bool(p.q(stored) and p.q("ws:" + n) >= 0), n
    for n in ("xin", "a", "arena", "gpre", "win0", "relw0", "gd", "health", "nonsense", ""):
        assert p.q("health_row:" + n) == -1, n
    if opts is UNFUSED or dt == 0:
        assert {"b0.qkv1", "b0.qkv2", "t1der"} <= set(names) and (("t2der" in names) == (scale == 4))
    elif dt == 1:
        assert "b0.qkv1" not in names and "b0.qkv2" not in names
    # the layout: the training regions where they were, the record behind them
    for n in all_names(nb, scale):
        assert p.q("ws:" + n) == plain.q("ws:" + n) and p.q("wsn:" + n) == plain.q("wsn:" + n), n
    assert p.q("ws:health") >= plain.q("workspace_bytes") and p.q("wsn:health") == (1 + len(names)) * 72
    chunks = sum(max(1, -(-(p.q("wsn:" + n) if n not in ("sr", "grads") else
                            (p.q("num_params") if n == "grads" else 2 * 3 * 40 * 56 * scale * scale)) // 32768)) for n in names)
    assert p.q("wsn:health_part") == chunks * 72
    assert p.q("workspace_bytes") >= p.q("ws:health_part") + 8 * p.q("wsn:health_part")


def test_a_later_option_moves_the_rows_before_initialisation(lib):
    p = P(lib, 1, 4, health=2)
    assert p.q("health_row:b0.qkv1") == -1 and p.q("health_row:t2der") == -1
    for k, v in UNFUSED.items():
        assert p.set(k, v) == 0
    assert p.q("health_row:b0.qkv1") > 0 and p.q("health_row:t2der") > 0 and p.q("health_row:g_t2pre") > 0
    assert _names(lib, p) == sum(_expected(p, 2), [])


def test_state_and_argument_rules_name_themselves(lib):
    train = P(lib, 1, 4)
    for bad in (-1, 3, 100):
        assert train.set("health", bad) == -2 and "health: 0 (off), 1" in _err(lib)
    for bad in (-1, 2):
        assert train.set("health_on", bad) == -2 and "health_on: 0 / 1" in _err(lib)
    lean = P(lib, 1, 4, inference=1)
    assert lean.set("health", 1) == -3 and "needs a training plan" in _err(lib) and "inference" in _err(lib)
    assert lean.set("health", 7) == -2                                                   # the argument rule comes first
    assert lean.set("health_on", 0) == -3 and "inference plan" in _err(lib)
    assert lean.q("health_rows") == 0 and lean.q("ws:health") == -1
    assert train.set("health", 2) == 0
    assert train.set("inference", 1) == -3 and "\"health\" > 0" in _err(lib)
    assert train.q("opt:inference") == 0 and train.q("opt:health") == 2
    assert train.set("inference", 0) == 0                                               # clearing what is clear is no refusal
    assert train.set("health", 0) == 0 and train.set("inference", 1) == 0


# ------------------------------------------------------------------------------------------------------------- the restatement
def test_the_restatement_by_hand():
    x = np.array([0.0, -0.0, 1.0, -3.0, 0.75, np.nan, np.inf, -np.inf, 2.0 ** -41, 2.0 ** -45, 2.0 ** 20, 2.0 ** 25, 1e-40], np.float32)
    r = R.row(x)
    assert r[0] == 13 and r[1] == 3 and r[2] == 1 and r[3] == 2.0 ** 25 and r[6] == 2 and r[7] == float(np.float32(1e-40))
    assert r[4] == float(np.sum(x[np.isfinite(x)].astype(np.float64))) and r[8] == 2 and r[8 + 63] == 3
    want = np.zeros(64)
    want[0], want[63] = 2, 3
    want[42] += 1                                     # 1.0: floor(log2) = 0
    want[43] += 1                                     # 3.0: 1
    want[41] += 1                                     # 0.75: -1
    want[1] += 3                                      # 2^-41, 2^-45 (clamped), the subnormal
    want[62] += 2                                     # 2^20, 2^25 (clamped)
    assert (r[8:] == want).all() and r[8:].sum() == r[0]
    e = R.row(np.zeros(0, np.float32))
    assert e[0] == 0 and e[3] == 0 and e[7] == np.inf and not e[8:].any()


# ------------------------------------------------------------------------------------------------------------- fp8 arithmetic
def _hist(**binades):
    h = np.zeros(64, np.int64)
    for k, v in binades.items():
        h[int(k[1:].replace("m", "-")) + 42 if k[0] == "e" else {"zeros": 0, "bad": 63}[k]] = v
    return h


def test_fp8_report_on_hand_worked_histograms():
    from m2trans_amd.health import HealthReport, fp8_shares
    # e4m3: top binade 8, normals down to -6, subnormals -7 .. -9.  absmax in binade 3 -> shift +5:
    #   binade 3 -> 8 normal; -11 -> -6 normal; -12 -> -7 sub; -14 -> -9 sub; -15 -> -10 flush
    h = _hist(e3=10, em11=20, em12=30, em14=25, em15=15, zeros=1000, bad=7)
    s = fp8_shares(h, "e4m3")
    assert s == {"normal": 0.30, "subnormal": 0.55, "flush": 0.15, "binades": 19, "e_max": 3}
    # e5m2: top binade 15, normals down to -14, subnormals -15, -16.  shift +12: -11 -> 1 ... all normal until binade -26 -> -14
    s = fp8_shares(h, "e5m2")
    assert s["normal"] == 1.0 and s["subnormal"] == 0.0 and s["flush"] == 0.0
    h2 = _hist(e0=1, em29=1, em30=1, em31=1, em32=1)  # e5m2 shift +15: -29 -> -14 normal, -30 -> -15 sub, -31 -> -16 sub, -32 -> -17 flush
    assert fp8_shares(h2, "e5m2") == {"normal": 0.4, "subnormal": 0.4, "flush": 0.2, "binades": 33, "e_max": 0}
    assert fp8_shares(_hist(zeros=5, bad=2), "e4m3") is None
    with pytest.raises(ValueError, match="e4m3"):
        fp8_shares(h, "e3m4")
    rec = np.zeros((3, 72))
    rec[0, :5] = (1, 1, -1, -1, 2)
    rec[1, 0], rec[1, 3], rec[1, 8:] = h.sum(), 9.5, h
    rec[1, 1] = 7
    rec[2, 0], rec[2, 3], rec[2, 8:] = h2.sum(), 1.5, h2
    rep = HealthReport(["a", "b"], [0, 1], rec)
    assert rep.fp8_report("e4m3")["a"]["flush"] == 0.15 and rep.fp8_report("e5m2")["b"]["subnormal"] == 0.4
    assert [r.name for r in rep.worst(1)] == ["a"] and rep["b"].phase == "backward" and "a" in rep and len(rep) == 2


def test_report_fields_first_nonfinite_and_log_line():
    from m2trans_amd.health import HealthReport
    x = np.array([1.0, -2.0, 0.0, np.nan, 4.0], np.float32)
    rec = np.zeros((4, 72))
    rec[0, :5] = (3, 2, -1, 2, 3)
    rec[1], rec[2], rec[3] = R.row(np.float32([0.5, 0.25])), R.row(np.float32([8.0])), R.row(x)
    rep = HealthReport(["sr", "X0", "gT"], [0, 0, 1], rec)
    assert rep.forward_passes == 3 and rep.backward_passes == 2
    r = rep["gT"]
    assert (r.n, r.nonfinite, r.nan, r.absmax, r.zeros, r.min_nonzero) == (5, 1, 1, 4.0, 1, 1.0)
    assert r.mean == 3.0 / 4 and r.rms == (21.0 / 4) ** 0.5 and r.hist.sum() == 5
    assert rep.first_nonfinite == ("backward", "gT")
    assert rep.log_line() == "health: non-finite first in backward row gT (1 of 5 elements, 1 NaN)"
    rec[0, 3] = -1
    clean = HealthReport(["sr", "X0", "gT"], [0, 0, 1], rec)
    assert clean.first_nonfinite is None and clean.log_line() == "health: absmax X0 8, gT 4, sr 0.5"
    rec[0, 2] = 1
    assert HealthReport(["sr", "X0", "gT"], [0, 0, 1], rec).first_nonfinite == ("forward", "X0")


# ------------------------------------------------------------------------------------------------------------- config, stub step
def test_train_config_takes_track_health_and_still_names_an_unknown_key():
    from m2trans_amd import train as T
    from m2trans_amd._lib import M2TError
    base = {"scale": 4, "patch_size": 96, "batch_size": 2, "epochs": 1, "lr": 1e-4, "eta_min": 1e-6, "log_every": 1, "test_every": 1,
            "training_dataset": "folder", "train_hr_path": "x"}
    assert "track_health" not in T.resolve_config(base)["train_step"]
    assert T.resolve_config(dict(base, track_health=50))["train_step"]["track_health"] == 50
    assert T.resolve_config(dict(base, track_health=0))["train_step"]["track_health"] == 0
    for bad in (-1, 2.5, True, "often"):
        with pytest.raises(M2TError, match="track_health"):
            T.resolve_config(dict(base, track_health=bad))
    with pytest.raises(M2TError, match="track_healht"):
        T.resolve_config(dict(base, track_healht=50))


def test_the_step_flips_the_switch_on_a_stub(monkeypatch):
    """TrainStep._health_switch on an object assembled without __init__ and a recording library: option "health_on" is set only when it
    changes, to 1 on the steps with step_count % K == 0 (the last micro-batch of an accumulation cycle), else to 0."""
    from m2trans_amd import _lib
    from m2trans_amd.train_step import TrainStep
    calls = []
    stub = types.SimpleNamespace(m2t_set_option=lambda h, k, v: calls.append((k, v)) or 0)
    ts = TrainStep.__new__(TrainStep)
    plan = types.SimpleNamespace(handle=None)
    ts.accum_steps, ts.micro_count, ts.step_count = 1, 0, 0
    ts._health_switch(stub, plan)
    assert calls == []                                          # track_health = 0 (the class default): nothing
    ts.track_health = 3
    seen = []
    for step in range(8):
        ts.step_count = step
        ts._health_switch(stub, plan)
        seen.append(plan.health_on if hasattr(plan, "health_on") else True)
    assert seen == [True, False, False, True, False, False, True, False]
    assert calls == [(b"health_on", 0), (b"health_on", 1), (b"health_on", 0), (b"health_on", 1), (b"health_on", 0)]
    ts.accum_steps, ts.step_count, calls[:] = 2, 3, []
    got = []
    for micro in (0, 1):
        ts.micro_count = micro
        ts._health_switch(stub, plan)
        got.append(plan.health_on)
    assert got == [False, True]
    with pytest.raises(_lib.M2TError, match="track_health"):
        TrainStep(None, track_health=-1)
    with pytest.raises(_lib.M2TError, match="track_health = 0"):
        ts2 = TrainStep.__new__(TrainStep)
        ts2.health()


def test_model_track_health_is_a_plain_attribute(monkeypatch):
    import copy
    from m2trans_amd import M2Trans_network as N
    from tests.gpu_util import make_args
    m = N.create_model(make_args(4, 1))
    assert m.health_level == 0 and m.track_health() is m and m.health_level == 2
    assert copy.deepcopy(m).health_level == 2
    with pytest.raises(N.M2TError, match="track_health"):
        m.track_health(3)
    with pytest.raises(N.M2TError, match="no forward"):
        m.health()
    made = []

    class FakePlan:
        def __init__(self, *a, **k):
            made.append(k)
            self.inference = k.get("inference", False)
    monkeypatch.setattr(N, "Plan", FakePlan)
    monkeypatch.setattr(N.M2Trans, "_device_ok", lambda self, x: None)
    monkeypatch.setattr(N.M2Trans, "_check_plan", lambda self, plan: None)
    x = types.SimpleNamespace(dim=lambda: 4, shape=(1, 3, 32, 32), device=types.SimpleNamespace(index=0))
    m._plan_for(x)
    m._plan_for(x, inference=True)
    m.track_health(0)
    m._plans.clear()
    m._plan_for(x)
    assert made == [{"options": {"health": 2}}, {"inference": True}, {}]


def test_timing_tool_host_part_runs_without_a_device():
    import importlib.util
    spec = importlib.util.spec_from_file_location("health_timing", os.path.join(ROOT, "tools", "health_timing.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args([])
    assert (a.batch, a.lr, a.n_blocks) == (16, 128, 8) and a.reps >= 50 and a.repeats >= 2
    assert tool.ARMS == ("off", "off_aa", "every", "k50", "switched")
    with pytest.raises(SystemExit):
        tool.parse_args(["--repeats", "1"])
    assert set(tool.RESULT_KEYS) >= {"step_ms", "aa_spread", "record_ms", "record_bytes", "copy_ms", "record_over_copy"}


# ------------------------------------------------------------------------------------------------------------- the kernel text on the host
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    # (clang: the header uses ext_vector_type and __bf16, as the device build does)
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"), shutil.which("clang++")) if c and os.path.exists(c)), None)
    assert cxx, "no clang-based C++ compiler found"
    exe = str(tmp_path_factory.mktemp("health") / "health_emulate")
    subprocess.run([cxx, "-x", "c++", "-std=c++20", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "tests", "emulate_hip"), "-I", os.path.join(ROOT, "m2trans_amd", "csrc"),
                    os.path.join(ROOT, "tests", "health_emulate.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def _emulate(exe, tmp_path, dtype, x, shift):
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<iiq", 1 if dtype == "bf16" else 0, shift, x.size) + np.ascontiguousarray(x, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return np.frombuffer(open(tmp_path / "out.bin", "rb").read(), dtype=np.float64)


def _to_bf16(x):
    """fp32 values truncated to the bf16 grid (representable in both element types)."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def adversarial(n, seed):
    """NaN, +-Inf, +-0, subnormals, both clamp ends of the histogram and every binade between, scattered over a Gaussian buffer."""
    rng = np.random.RandomState(seed)
    x = _to_bf16(rng.standard_normal(n).astype(np.float32) * np.float32(2.0) ** rng.randint(-50, 30, n).astype(np.float32))
    special = np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0, 2.0 ** -130, -2.0 ** -133, 2.0 ** -41, 1.5 * 2.0 ** -42, 2.0 ** -42, 2.0 ** 20,
                          1.75 * 2.0 ** 19, 2.0 ** 21, -3.0e38, 2.0 ** -126, 1.0, -1.0])
    if n >= 4 * special.size:
        where = rng.choice(n, 4 * special.size, replace=False)
        x[where] = np.tile(special, 4)
        x[n - 1], x[0] = np.nan, -np.inf              # the row's first and last element
    return _to_bf16(x)


@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
@pytest.mark.parametrize("n,shift", ((100003, 0), (100003, 3), (32768, 0), (32769, 1), (65541, 5), (7, 0), (5, 2), (0, 0), (2049, 7)))
def test_the_kernel_text_on_the_host_matches_the_restatement(emulator, tmp_path, n, shift, dtype):
    x = adversarial(n, seed=n + shift)
    got = _emulate(emulator, tmp_path, dtype, x, shift)
    R.compare(got, x, (n, shift, dtype))
    assert got[8:].sum() == n and got[8] == got[6] and got[8 + 63] == got[1]


def test_the_fold_does_not_depend_on_alignment_and_black_counts_as_zeros(emulator, tmp_path):
    x = adversarial(70001, seed=5)
    a, b = _emulate(emulator, tmp_path, "bf16", x, 0), _emulate(emulator, tmp_path, "bf16", x, 3)
    assert a.tobytes() == b.tobytes()                 # 16-byte loads or the plain loop: the same elements in the same order
    z = _emulate(emulator, tmp_path, "fp32", np.zeros(40000, np.float32), 0)
    assert z[0] == z[6] == z[8] == 40000 and z[3] == 0 and z[7] == np.inf and not z[[1, 2, 4, 5]].any()
