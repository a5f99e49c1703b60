"""CPU tests (no GPU) of option "local_norm" (include/m2t.h): the numpy restatement of the definition (tests/local_norm_ref.py), the
option's range and state rules, the workspace regions it adds to an inference plan, the Python / command-line / yaml surface, and
that the gate of tests/test_gpu_local_norm.py sees one-line faults.

Host-only calls, as in tests/test_lean_plan_cpu.py: m2t_plan_create / m2t_set_option / m2t_plan_query allocate nothing on a device.
Every test here fails without the feature: the option (or the module under test) does not exist there."""
import copy
import pickle
import types

import numpy as np
import pytest
import torch

from oracle import m2trans_oracle as O
from tests import local_norm_ref as R
from tests.test_lean_plan_cpu import P, all_names

ERR_ARG, ERR_STATE = -2, -3
STAGE_T = (24, 33, 64, 200)          # on the 64 x 64 plane: even, odd, the plane, clipped


@pytest.fixture(scope="module")
def lib():
    from m2trans_amd import _lib
    from tests.test_plan_surface_cpu import load_library
    return load_library(_lib.LIB_PATH)


def LN(lib, dt, scale, T, **kw):
    """An inference plan with local_norm = T (the option is legal only once "inference" is 1, so it is set last)."""
    p = P(lib, dt, scale, inference=1, **kw)
    assert p.set("local_norm", T) == 0
    return p


@pytest.fixture(scope="module")
def plane():
    return R.stage_plane(2, 3, 64, 64, seed=1)


# ------------------------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("T", STAGE_T + (8,))
def test_the_two_restatements_agree(plane, T):
    a, b = R.local_stats_brute(plane, T), R.local_stats_cumsum(plane, T)
    for name, u, v in zip("mvr", a, b):
        scale = 1.0 if name != "r" else np.abs(v)          # r reaches 316 over the black half-plane: relative there
        assert float(np.max(np.abs(u - v) / scale)) <= 1e-12, name
    xa, xb = R.local_norm_exact(plane, T, stats=R.local_stats_brute)[0], R.local_norm_exact(plane, T)[0]
    assert float(np.max(np.abs(xa - xb))) <= 1e-12 * float(np.max(np.abs(xb)))


def test_a_rectangular_plane_is_global_in_rows_and_local_in_columns():
    x = R.stage_plane(1, 2, 64, 96, seed=2)
    m, v, r = R.local_stats_brute(x, 80)
    assert np.all(m == m[:, :, :1, :])                       # k_h = 64 = the side: one window for every row
    assert not np.all(m == m[:, :, :, :1])
    m2 = R.local_stats_cumsum(x, 80)[0]
    assert float(np.max(np.abs(m - m2))) <= 1e-12


@pytest.mark.parametrize("T", (64, 65, 200, 16384))
def test_a_window_of_the_plane_is_the_global_instance_norm(plane, T):
    want = O.instance_norm(torch.from_numpy(plane)).numpy()
    got = R.local_norm_exact(plane, T)[0]
    assert float(np.max(np.abs(got - want))) <= 1e-12 * max(1.0, float(np.max(np.abs(want))))
    got_b = R.local_norm_exact(plane, T, stats=R.local_stats_brute)[0]
    assert float(np.max(np.abs(got_b - want))) <= 1e-12 * max(1.0, float(np.max(np.abs(want))))


def test_the_window_rule_by_hand():
    # k = 4 (even) on n = 10: left pad 1, right pad 2
    assert [R.window_start(y, 4, 10) for y in range(10)] == [0, 0, 1, 2, 3, 4, 5, 6, 6, 6]
    # k = 5 (odd): pads 2 and 2
    assert [R.window_start(y, 5, 10) for y in range(10)] == [0, 0, 0, 1, 2, 3, 4, 5, 5, 5]
    # k = n: one window
    assert {R.window_start(y, 10, 10) for y in range(10)} == {0}
    # the same from the statistics: a plane whose value is its column index; the mean of a window is start + (k - 1) / 2
    x = np.tile(np.arange(10.0), (1, 1, 10, 1))
    for k, starts in ((4, [0, 0, 1, 2, 3, 4, 5, 6, 6, 6]), (5, [0, 0, 0, 1, 2, 3, 4, 5, 5, 5])):
        for stats in (R.local_stats_brute, R.local_stats_cumsum):
            m = stats(x, k)[0]
            assert np.allclose(m[0, 0, 3], np.array(starts) + (k - 1) / 2.0, rtol=0, atol=1e-12), (k, stats.__name__)
    # rows likewise
    xt = np.tile(np.arange(10.0)[:, None], (1, 1, 1, 10))
    assert np.allclose(R.local_stats_brute(xt, 4)[0][0, 0, :, 7], np.array([0, 0, 1, 2, 3, 4, 5, 6, 6, 6]) + 1.5, rtol=0, atol=1e-12)


def test_the_definition_rounds_where_it_says(plane):
    xn32, xnbf = R.local_norm(plane, 24, "fp32"), R.local_norm(plane, 24, "bf16")
    assert xn32.dtype == np.float32 and xnbf.dtype == np.float32
    assert np.array_equal(xnbf, torch.from_numpy(xn32).to(torch.bfloat16).float().numpy())
    m, _, r = R.local_stats_cumsum(plane, 24)
    d = plane.astype(np.float32) - m.astype(np.float32)
    assert np.array_equal(xn32, d * r.astype(np.float32))
    black = R.local_norm(np.zeros((1, 2, 32, 32)), 24, "bf16")
    assert not black.any() and not np.signbit(black).any()


# ---------------------------------------------------------------------------------------------------------------- option and plan
def test_the_option_exists_reads_back_and_keeps_its_range(lib):
    p = P(lib, 1, 4, inference=1)
    assert p.q("opt:local_norm") == 0
    for T in (8, 24, 96, 16384):
        assert p.set("local_norm", T) == 0 and p.q("opt:local_norm") == T
    assert p.set("local_norm", 0) == 0 and p.q("opt:local_norm") == 0
    err = lambda: lib.m2t_last_error_string().decode()
    for bad in (-1, 1, 7, 16385, 1 << 40):
        assert p.set("local_norm", bad) == ERR_ARG and "local_norm" in err(), bad
        assert p.q("opt:local_norm") == 0


def test_state_rules(lib):
    err = lambda: lib.m2t_last_error_string().decode()
    train = P(lib, 1, 4)
    assert train.set("local_norm", 24) == ERR_STATE and "inference" in err()
    assert train.q("opt:local_norm") == 0 and train.q("ws:xn") == -1
    assert train.set("local_norm", 3) == ERR_ARG                          # the range answers before the state
    p = P(lib, 1, 4, inference=1)
    assert p.set("local_norm", 24) == 0
    assert p.set("inference", 0) == ERR_STATE and "local_norm" in err()
    assert p.q("opt:inference") == 1 and p.q("opt:local_norm") == 24
    assert p.set("inference", 1) == 0                                     # (setting it again is no change)
    assert p.set("local_norm", 0) == 0 and p.set("inference", 0) == 0 and p.q("opt:inference") == 0
    # (the rule "only before the first m2t_plan_init_workspace" needs a device: tests/test_gpu_local_norm.py)


@pytest.mark.parametrize("dt", (0, 1))
@pytest.mark.parametrize("nb", (1, 2, 3))
def test_regions_of_a_local_norm_plan(lib, dt, nb):
    B, H0, W0 = 2, 40, 56
    es = 2 if dt else 4
    lean, ln = P(lib, dt, 4, nb=nb, inference=1), LN(lib, dt, 4, 24, nb=nb)
    BP = B * 64 * 64
    assert [lean.q(f"{f}:{n}") for n in ("xn", "lnsum", "norm_id") for f in ("ws", "wsn")] == [-1] * 6
    assert (ln.q("wsn:xn"), ln.q("wsn:lnsum"), ln.q("wsn:norm_id")) == (BP * 64, BP * 64 * 2, B * 64 * 2)
    new = {"xn": BP * 64 * es, "lnsum": BP * 64 * 2 * 8, "norm_id": B * 64 * 2 * 4}
    # everything the lean plan has is where it was; the new regions follow, aligned, without overlap, up to workspace_bytes
    names = [n for n in all_names(nb, 4) if lean.q("ws:" + n) >= 0]
    assert names and [(ln.q("ws:" + n), ln.q("wsn:" + n)) for n in names] == [(lean.q("ws:" + n), lean.q("wsn:" + n)) for n in names]
    end = lean.q("workspace_bytes")
    for n in ("xn", "lnsum", "norm_id"):
        assert ln.q("ws:" + n) == end and end % 256 == 0, n
        end = (end + new[n] + 255) // 256 * 256
    assert ln.q("workspace_bytes") == end
    # the last block's input is a buffer of its own: nothing the forward writes after it aliases it
    xs = [ln.q(f"ws:X{b}") for b in range(nb + 1)]
    assert xs[nb - 1] not in xs[nb:] and ln.q("ws:xn") not in xs
    # clearing the option gives the lean plan back
    assert ln.set("local_norm", 0) == 0
    keys = ["workspace_bytes"] + [f"{f}:{n}" for n in all_names(nb, 4) + ["xn", "lnsum", "norm_id"] for f in ("ws", "wsn")]
    assert [ln.q(k) for k in keys] == [lean.q(k) for k in keys]


@pytest.mark.parametrize("dt", (0, 1))
@pytest.mark.parametrize("scale", (2, 3, 4))
def test_plans_without_the_option_are_untouched(lib, dt, scale):
    """Setting the option and clearing it again leaves a lean plan as a fresh one; a default plan never sees it; opt: keys of other
    options are what they were."""
    opts = ("inference", "fused_tail", "attn_bwd", "fused_attn_fwd", "fused_c16_fwd", "fused_prep_fwd", "side_stream", "conv_rows",
            "fused_attn_fwd2", "fp32_fast", "gate_branch", "wgrad_big_tiles")
    keys = ["workspace_bytes", "stores_qkv1", "stores_qkv2", "stores_t1", "stores_t2"] + ["opt:" + k for k in opts]
    keys += [f"{f}:{n}" for n in all_names(2, scale) for f in ("ws", "wsn")]
    fresh, back = P(lib, dt, scale, inference=1), P(lib, dt, scale, inference=1)
    assert back.set("local_norm", 96) == 0 and back.q("workspace_bytes") > fresh.q("workspace_bytes")
    assert [back.q(k) for k in keys if k != "workspace_bytes"] == [fresh.q(k) for k in keys if k != "workspace_bytes"]
    assert back.set("local_norm", 0) == 0
    assert [back.q(k) for k in keys] == [fresh.q(k) for k in keys]
    train, train2 = P(lib, dt, scale), P(lib, dt, scale)
    assert train2.set("local_norm", 96) == ERR_STATE
    assert [train2.q(k) for k in keys] == [train.q(k) for k in keys] and train.q("opt:local_norm") == 0


def test_workspace_bytes_of_default_and_lean_plans_are_the_recorded_ones(lib):
    """(1, 512, 512), x4, bf16, 8 blocks: the two figures README.md and INTEGRATION.md have carried since the inference plan
    (5.54 GB and 0.373 GB), to three digits."""
    shape = (1, 512, 512)
    assert round(P(lib, 1, 4, shape, nb=8).q("workspace_bytes") / 1e9, 2) == 5.54
    assert round(P(lib, 1, 4, shape, nb=8, inference=1).q("workspace_bytes") / 1e9, 3) == 0.373


# ------------------------------------------------------------------------------------------------------------ Python, CLI, yaml
def _model(**extra):
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=2, rgb_range=1.0, n_blocks=1, colors=3, compute_dtype="bf16", **extra))


def test_model_local_norm_is_a_plain_attribute_and_implies_lean():
    from m2trans_amd._lib import M2TError
    m = _model()
    assert m.local_norm_window == 0 and m.lean_inference_enabled is False
    assert m.local_norm(24) is m and m.local_norm_window == 24 and m.lean_inference_enabled is True
    assert copy.deepcopy(m).local_norm_window == 24 and copy.deepcopy(m).lean_inference_enabled is True
    assert pickle.loads(pickle.dumps(m)).local_norm_window == 24
    assert m.__dict__["local_norm_window"] == 24            # rides along in the shallow copy nn.DataParallel makes
    assert m.local_norm(0) is m and m.local_norm_window == 0 and m.lean_inference_enabled is True
    assert m.local_norm(None).local_norm_window == 0
    assert copy.deepcopy(m).local_norm_window == 0
    for bad in (7, -3, 16385):
        with pytest.raises(M2TError, match="local_norm"):
            m.local_norm(bad)
    assert _model(local_norm=96).local_norm_window == 96 and _model(local_norm=96).lean_inference_enabled is True
    assert "train global, test local" in type(m).local_norm.__doc__


def test_local_norm_plans_have_their_own_cache_key(monkeypatch):
    from m2trans_amd import M2Trans_network as N
    made = []

    class FakePlan:
        def __init__(self, B, H0, W0, scale, n_blocks, dtype, device, inference=False, local_norm=0):
            self.inference, self.local_norm = inference, local_norm
            made.append((inference, local_norm))

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
    c, d = m._plan_for(X(), inference=True, local_norm=24), m._plan_for(X(), local_norm=96)
    assert len({id(p) for p in (a, b, c, d)}) == 4 and made == [(False, 0), (True, 0), (True, 24), (True, 96)]
    assert m._plan_for(X(), local_norm=24) is c and m._plan_for(X(), inference=True) is b and len(m._plans) == 4
    assert {k[5:] for k in m._plans} == {(), ("inference",), ("local_norm", 24), ("local_norm", 96)}      # (the cache is in LRU order)


def test_forward_picks_the_plan_of_the_setting(monkeypatch):
    from m2trans_amd import M2Trans_network as N
    asked = []
    monkeypatch.setattr(N.M2Trans, "_plan_for", lambda self, x, inference=False, local_norm=0: asked.append((inference, local_norm)))
    monkeypatch.setattr(N.M2Trans, "_run_forward", lambda self, plan, x, keep, want_sr=True: None)
    m = _model()
    x = torch.zeros(1, 3, 32, 32)
    with torch.no_grad():
        m(x); m.local_norm(24); m(x); m.local_norm(0); m(x); m.lean_inference(False); m(x)
    assert asked == [(False, 0), (True, 24), (True, 0), (False, 0)]


def test_train_config_takes_local_norm():
    from m2trans_amd import train as T
    from m2trans_amd._lib import M2TError
    cfg = {"scale": 2, "patch_size": 64, "batch_size": 4, "epochs": 1, "lr": 1e-4, "eta_min": 1e-6, "log_every": 1, "test_every": 1,
           "data_path": "/nowhere", "lambda_clip": 0}
    assert "local_norm" in T.MODEL_KEYS and "local_norm" in T.REFERENCE_KEYS
    assert "local_norm" not in T.resolve_config(cfg)["model"]
    r = T.resolve_config(dict(cfg, local_norm=96))
    assert r["model"]["local_norm"] == 96 and "local_norm" not in r["train_step"] and "local_norm" not in r["fit"]
    for bad in ("96", True, 7, 96.0, 20000):
        with pytest.raises(M2TError, match="local_norm"):
            T.resolve_config(dict(cfg, local_norm=bad))
    with pytest.raises(M2TError, match="local_norms"):                    # an unknown key is still named
        T.resolve_config(dict(cfg, local_norms=96))
    from m2trans_amd.infer import model_namespace
    from m2trans_amd.M2Trans_network import create_model
    m = create_model(model_namespace(dict(r["model"], n_blocks=1)))
    assert m.local_norm_window == 96 and m.lean_inference_enabled is True


def test_infer_cli_parses_local_norm():
    import inspect
    from m2trans_amd import infer
    base = ["--config", "c.yml", "--model_path", "m.pt", "--input", "in", "--output", "out"]
    assert infer.parse_args(base).local_norm is None
    assert infer.parse_args(base + ["--local_norm", "96"]).local_norm == 96
    a = infer.parse_args(base + ["--local_norm", "144", "--self_ensemble", "--tile", "64"])
    assert a.local_norm == 144 and a.tile == 64
    for bad in ("7", "0", "16385", "x"):
        with pytest.raises(SystemExit):
            infer.parse_args(base + ["--local_norm", bad])
    assert inspect.signature(infer.upscale_folder).parameters["local_norm"].default is None


def test_timing_tool_host_part_runs_without_a_device():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("local_norm_timing", os.path.join(root, "tools", "local_norm_timing.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args([])
    assert (a.lr, a.scale, a.n_blocks, a.dtype) == (512, 4, 8, "bf16") and a.reps >= 1 and a.repeats >= 2
    assert tool.ARMS == ("plain", "plain_again", "local_96", "local_144", "tiled_128_16")
    with pytest.raises(SystemExit):
        tool.parse_args(["--reps", "0"])
    assert set(tool.RESULT_KEYS) >= {"ms", "aa_spread", "workspace_bytes", "psnr_db", "bytes_per_element_and_block"}


# ------------------------------------------------------------------------------------------------------------ the gate sees faults
GATE_CASES = tuple((64, 64, T) for T in STAGE_T) + ((64, 96, 80),)


@pytest.fixture(scope="module")
def gate_planes():
    return {(H, W): R.stage_plane(1, 4, H, W, seed=3) for H, W in {(64, 64), (64, 96)}}


@pytest.mark.parametrize("H,W,T", GATE_CASES)
@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_the_unfaulted_restatement_passes_on_every_element(gate_planes, H, W, T, dtype):
    x = gate_planes[(H, W)]
    if dtype == "bf16":
        x = R.round_bf16(x.astype(np.float32)).astype(np.float64)
    for stats in (R.local_stats_cumsum, R.local_stats_brute):
        nbad, worst = R.gate(R.local_norm(x, T, dtype, stats=stats), x, T, dtype)
        assert nbad == 0 and worst <= 1.0, (stats.__name__, nbad, worst)


# where each fault shows: a window-placement fault needs an even k with room to move (T = 24; at odd k the two pads are equal and the
# swapped-pad window IS the right one), the count fault needs T beyond the side, the others show everywhere
FAULT_CASES = {"start_half": ((64, 64, 24), (64, 96, 80)), "pads_swapped": ((64, 64, 24), (64, 96, 80)),
               "unbiased": GATE_CASES, "no_eps": GATE_CASES, "k_unclipped": ((64, 64, 200), (64, 96, 80)),
               "shift_col": ((64, 64, 24), (64, 64, 33), (64, 96, 80))}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_gate_sees_each_one_line_fault(gate_planes, fault):
    """In the fp32 gate.  (In bf16 the output rounding, 2^-8 relative, is wider than the unbiased-variance fault at n = 576, which
    moves xn by 1 / (2 n) = 8.7e-4 relative: the bf16 stage test of the device cannot see that one fault, the fp32 one does.)"""
    assert set(FAULT_CASES) == set(R.FAULTS)
    for H, W, T in FAULT_CASES[fault]:
        x = gate_planes[(H, W)]
        nbad, worst = R.gate(R.local_norm(x, T, "fp32", fault=fault), x, T, "fp32")
        assert nbad > 0 and worst > 1.0, (fault, T, nbad, worst)
    if fault in ("start_half", "pads_swapped"):              # odd k: the same window, and the gate says so
        x = gate_planes[(64, 64)]
        assert R.gate(R.local_norm(x, 33, "fp32", fault=fault), x, 33, "fp32")[0] == 0
