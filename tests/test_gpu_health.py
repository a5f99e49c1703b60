"""GPU tests of the step health record (option "health" of include/m2t.h; csrc/k_health.hip): every row against the restatement
tests/health_ref.py on the workspace views read back after the pass, the location of a NaN / Inf planted in DATA (ordinary floats:
nothing here faults a device), reproducibility, and that the record only reads.

Shape: B = 2, LR 3 x 40 x 56 (pads to 64 x 64, non-square); one and two blocks, x2 and x4, bf16 and fp32, the default options and the
unfused ones (so that q | k | v, gelu' and the plain tail's gradients have rows).  Tolerances: slots 0 - 3, 6, 7 and the 64 bins are
equal; slots 4 and 5 are within n * 2^-53 * sum |x| and n * 2^-53 * sum x^2 of the restatement (health_ref.sum_bounds: derived).
"""
import pytest
import torch

from tests import health_ref as R

pytestmark = pytest.mark.gpu

B, H0, W0 = 2, 40, 56
UNFUSED = {"fused_attn_fwd": 0, "fused_c16_fwd": 0, "fused_tail": 0}
CASES = ((4, 1, "bf16", False), (4, 2, "bf16", True), (2, 2, "bf16", False), (4, 1, "fp32", False), (2, 2, "fp32", False))


def _setup(scale, nb, dtype, unfused=False, level=2, **opts):
    """A model whose training plan of the test shape carries the record and the given options (set before the workspace is laid out)."""
    from m2trans_amd import _lib
    from m2trans_amd.M2Trans_network import Plan
    from tests.gpu_util import build_model
    model, _ = build_model(scale, nb, dtype)
    options = dict(UNFUSED if unfused else {}, **opts)
    if level:
        options["health"] = level
    dev = model.flat_params.device
    code = _lib.F32 if dtype == "fp32" else _lib.BF16
    plan = Plan(B, H0, W0, scale, nb, code, dev, options=options)
    model._plans[(B, H0, W0, code, dev.index)] = plan
    return model, plan


def _images(scale, seed=0):
    from oracle import m2trans_oracle as O
    x = O.closed_form_image(B, 3, H0, W0).cuda()
    g = torch.Generator().manual_seed(seed)
    g_sr = (torch.randn(B, 3, H0 * scale, W0 * scale, generator=g) * 1e-3).cuda()
    return x, g_sr


def _step(model, plan, x, g_sr):
    """forward, seed, backward through the C ABI; returns (sr, grads)."""
    from m2trans_amd import _lib
    lib = _lib.load()
    assert model._plan_for(x) is plan
    sr = model._run_forward(plan, x, keep=True)
    grads = torch.empty_like(model.flat_params)
    st, ws = _lib.stream_ptr(), _lib.ptr(plan.workspace)
    _lib.check(lib.m2t_set_output_grad(plan.handle, _lib.ptr(g_sr), float(model.rgb_range), ws, st), "m2t_set_output_grad")
    _lib.check(lib.m2t_backward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(x), _lib.ptr(grads), ws, st), "m2t_backward")
    torch.cuda.synchronize()
    return sr, grads


def _tensor(plan, name, sr, grads):
    if name == "sr":
        return sr
    if name == "grads":
        return grads
    f32 = name == "srpre" or name.endswith((".mean", ".rstd"))
    return plan.ws_tensor(name, dtype=torch.float32 if f32 else None)


def _check_rows(report, plan, sr, grads):
    worst = 0.0
    for r in report:
        ratios = R.compare(report.record[1 + plan.query("health_row:" + r.name)], _tensor(plan, r.name, sr, grads), r.name)
        worst = max(worst, *ratios)
    return worst


_RUNS = {}


def _run(case):
    """One step per case, shared by the tests that only read it."""
    if case not in _RUNS:
        from m2trans_amd.health import HealthReport
        scale, nb, dtype, unfused = case
        model, plan = _setup(scale, nb, dtype, unfused)
        x, g_sr = _images(scale)
        sr, grads = _step(model, plan, x, g_sr)
        _RUNS[case] = (model, plan, x, g_sr, sr, grads, HealthReport.from_plan(plan))
    return _RUNS[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"x{c[0]}-{c[1]}blk-{c[2]}-{'unfused' if c[3] else 'default'}")
def test_every_row_against_the_restatement(case):
    model, plan, x, g_sr, sr, grads, rep = _run(case)
    assert rep.forward_passes == 1 and rep.backward_passes == 1 and rep.first_nonfinite is None
    assert int(rep.record[0, 4]) == len(rep) == plan.query("health_rows") and not rep.record[0, 5:].any()
    names = [r.name for r in rep]
    assert names[0] == "sr" and names[-1] == "grads" and [r.phase for r in rep] == sorted((r.phase for r in rep), reverse=True) and "gT" in names
    if case[3] or case[2] == "fp32":
        assert {"b0.qkv1", "b0.qkv2", "t1der", "g_t1pre"} <= set(names)
    worst = _check_rows(rep, plan, sr, grads)
    print(f"health rows {len(rep)}, worst sum error / bound {worst:.3g}")
    assert rep["sr"].n == sr.numel() and rep["grads"].n == grads.numel() and rep["X0"].n == B * 64 * 64 * 64
    assert rep["sr"].absmax <= 1.0 and rep["grads"].nonfinite == 0
    shares = rep.fp8_report("e4m3")["gT"]
    assert abs(shares["normal"] + shares["subnormal"] + shares["flush"] - 1.0) < 1e-12


def test_rules_of_an_initialised_plan():
    from m2trans_amd import _lib
    lib = _lib.load()
    model, plan, *_ = _run(CASES[0])
    err = lambda: lib.m2t_last_error_string().decode()
    assert lib.m2t_set_option(plan.handle, b"health", 1) == -3 and "before the first m2t_plan_init_workspace" in err()
    assert lib.m2t_set_option(plan.handle, b"health", 5) == -2
    for k in (b"fused_tail", b"attn_bwd", b"fused_attn_fwd", b"fused_c16_fwd"):
        assert lib.m2t_set_option(plan.handle, k, 0) == -3 and "rows of the health record" in err(), k
    assert lib.m2t_set_option(plan.handle, b"inference", 1) == -3
    assert lib.m2t_set_option(plan.handle, b"health_on", 0) == 0 and plan.query("opt:health_on") == 0
    assert lib.m2t_set_option(plan.handle, b"health_on", 1) == 0 and plan.query("opt:health_on") == 1


def test_a_nan_pixel_is_located_at_the_head():
    from m2trans_amd.health import HealthReport
    model, plan = _setup(4, 1, "bf16")
    x, g_sr = _images(4)
    x[1, 2, 17, 23] = float("nan")
    sr, grads = _step(model, plan, x, g_sr)
    rep = HealthReport.from_plan(plan)
    assert rep.first_nonfinite == ("forward", "X0")          # sr is clamped: the first row that depends on the input is the head's
    # the 3 x 3 head conv spreads the pixel over 9 positions x 64 channels -- twice: the reflect pad mirrors row 17 into row 61
    assert rep["sr"].nonfinite == 0 and rep["X0"].nan == rep["X0"].nonfinite == 2 * 9 * 64
    _check_rows(rep, plan, sr, grads)                          # every count exact


def test_a_nan_weight_of_block_1_leaves_block_0_clean():
    from m2trans_amd.health import HealthReport
    model, plan = _setup(4, 2, "bf16")
    x, g_sr = _images(4)
    with torch.no_grad():
        model.body[1].attn1.qkv_conv.weight.view(-1)[5] = float("nan")
    sr, grads = _step(model, plan, x, g_sr)
    rep = HealthReport.from_plan(plan)
    for r in rep:
        if r.phase == "forward" and (r.name.startswith("b0.") or r.name in ("sr", "X0", "X1")):
            assert r.nonfinite == 0, r
    phase, name = rep.first_nonfinite
    assert phase == "forward" and name.startswith("b1."), name
    assert rep["X2"].nonfinite > 0
    _check_rows(rep, plan, sr, grads)


def test_an_inf_in_the_seed_is_a_backward_row():
    from m2trans_amd.health import HealthReport
    model, plan = _setup(4, 1, "bf16")
    x, g_sr = _images(4)
    g_sr[0, :, 40:48, :] = float("inf")
    sr, grads = _step(model, plan, x, g_sr)
    rep = HealthReport.from_plan(plan)
    assert all(r.nonfinite == 0 for r in rep if r.phase == "forward")
    assert rep.first_nonfinite is not None and rep.first_nonfinite[0] == "backward" and int(rep.record[0, 2]) == -1
    assert rep.first_nonfinite[1] == next(r.name for r in rep if r.phase == "backward" and r.nonfinite > 0)
    _check_rows(rep, plan, sr, grads)


def test_black_input_reproducibility_and_a_poisoned_workspace():
    from m2trans_amd import _lib
    from m2trans_amd.health import HealthReport
    model, plan = _setup(4, 2, "bf16")
    x, g_sr = _images(4)
    sr, grads = _step(model, plan, torch.zeros_like(x), g_sr)
    rep = HealthReport.from_plan(plan)
    _check_rows(rep, plan, sr, grads)                          # a black input: the zero counts the restatement gives
    first = _step(model, plan, x, g_sr) and HealthReport.from_plan(plan).record.copy()
    again = _step(model, plan, x, g_sr) and HealthReport.from_plan(plan).record.copy()
    assert first[0, 0] == 2 and again[0, 0] == 3 and again[0, 1] == 3
    assert first[1:].tobytes() == again[1:].tobytes() and first[0, 2:].tobytes() == again[0, 2:].tobytes()
    plan.workspace.fill_(0xFF)                                 # NaN in every element type, the record and its tables included
    _lib.check(_lib.load().m2t_plan_init_workspace(plan.handle, _lib.ptr(plan.workspace), _lib.stream_ptr()), "m2t_plan_init_workspace")
    _step(model, plan, x, g_sr)
    fresh = HealthReport.from_plan(plan).record
    assert fresh[0, 0] == 1 and fresh[0, 1] == 1 and fresh[1:].tobytes() == first[1:].tobytes()


def _two_steps(level, on, side):
    from m2trans_amd import _lib
    from m2trans_amd.train_step import TrainStep
    model, plan = _setup(4, 2, "bf16", level=level, side_stream=side)
    if not on:
        _lib.check(_lib.load().m2t_set_option(plan.handle, b"health_on", 0), "health_on")
    x, _ = _images(4)
    from oracle import m2trans_oracle as O
    hr = O.closed_form_image(B, 3, H0 * 4, W0 * 4, phase=0.7).cuda()
    sr = model._run_forward(plan, x, keep=True).clone()
    ts = TrainStep(model, lr=1e-3, world_size=1)
    out = [sr]
    for _ in range(2):
        loss = ts.step(x, hr)
        out += [loss.clone(), ts.grads.clone()]
    out.append(model.flat_params.clone())
    torch.cuda.synchronize()
    head = plan.ws_tensor("health", (-1, 72), torch.float64)[0, :2].tolist() if level else None
    return out, head


def test_the_record_only_reads():
    """sr, the loss and every gradient of two TrainStep steps and the parameters after them: bit-identical whatever the record does."""
    base, _ = _two_steps(0, True, 1)
    for level in (0, 1, 2):
        for on in (True, False):
            for side in (0, 1):
                got, head = _two_steps(level, on, side)
                for i, (a, b) in enumerate(zip(base, got)):
                    assert torch.equal(a, b), (level, on, side, i)
                if level:
                    # (one forward of the test's own, then two steps) -- or nothing at all with the switch off
                    assert head == ([3.0, 2.0 if level == 2 else 0.0] if on else [0.0, 0.0]), (level, on, side, head)


def test_track_health_3_records_steps_0_3_and_6():
    from m2trans_amd.train_step import TrainStep
    from oracle import m2trans_oracle as O
    from tests.gpu_util import build_model
    model, _ = build_model(4, 1, "bf16")
    x, _ = _images(4)
    hr = O.closed_form_image(B, 3, H0 * 4, W0 * 4, phase=0.7).cuda()
    model(x)                                                   # a training-shape plan without a record would be in the way: dropped
    with torch.no_grad():
        model(x)
    ts = TrainStep(model, lr=1e-4, world_size=1, track_health=3, skip_nonfinite=True)
    counts = []
    for _ in range(7):
        ts.step(x, hr)
        torch.cuda.synchronize()
        counts.append(tuple(ts._last_plan.ws_tensor("health", (-1, 72), torch.float64)[0, :2].tolist()))
    assert counts == [(1, 1), (1, 1), (1, 1), (2, 2), (2, 2), (2, 2), (3, 3)]
    rep = ts.health()
    assert rep.first_nonfinite is None and rep.backward_passes == 3 and rep["grads"].n == model.flat_params.numel()
    assert [r.name for r in rep.worst(3)] == [r.name for r in sorted(rep, key=lambda r: -r.absmax)[:3]]
    assert model.health() is not None and int(ts.skipped_steps.item()) == 0


def test_fit_writes_the_health_line(tmp_path):
    from tests.test_gpu_train import _fit, _objects
    r = _fit(tmp_path, objects=_objects(track_health=1), epochs=1, test_every=5, preview_every=100)
    lines = [l for l in r["lines"] if l.startswith("health: ")]
    assert len(lines) == 3 and all(l.startswith("health: absmax ") for l in lines), r["lines"]
