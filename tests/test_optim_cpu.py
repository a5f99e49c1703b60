"""CPU tests (no GPU) of the optimizer options of TrainStep -- gradient-norm clipping, weight decay, EMA weights, the non-finite
skip: the interface from the constructor down to the exported symbols, the yardstick of tests/optim_ref.py against torch's own
Adam, the checkpoint format with the options on and off, and the host part of tools/optim_timing.py."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"max_grad_norm": None, "weight_decay": 0.0, "decoupled_weight_decay": False, "ema_decay": None,
            "skip_nonfinite": False, "track_grad_norm": False}


def test_interface_reaches_from_the_constructor_to_the_exported_symbols():
    from m2trans_amd import _lib
    from m2trans_amd.train_step import TrainStep
    par = inspect.signature(TrainStep.__init__).parameters
    for k, d in DEFAULTS.items():
        assert k in par and par[k].default == d and type(par[k].default) is type(d), k
    vp, ll, f, i = C.c_void_p, C.c_longlong, C.c_float, C.c_int
    assert _lib.ABI["m2t.h"]["m2t_grad_norm"] == (i, [vp, ll, f, f, i, i, f, f, vp, vp, vp])
    assert _lib.ABI["m2t.h"]["m2t_grad_norm_workspace_bytes"] == (ll, [])
    assert _lib.ABI["m2t.h"]["m2t_adam_step_ex"] == (i, [vp, vp, vp, vp, ll, f, f, f, f, i, f, vp, f, i, f, vp, vp])
    hdr = open(os.path.join(ROOT, "include", "m2t.h")).read()
    assert re.search(r"\bint\s+m2t_grad_norm\s*\(\s*const float\*\s*grads,\s*long long n,\s*float grad_scale,\s*float max_norm,"
                     r"\s*int skip_nonfinite,\s*int step,\s*float beta1,\s*float beta2,\s*double\*\s*record,\s*void\*\s*workspace,"
                     r"\s*void\*\s*stream\)", hdr)
    assert re.search(r"\blong long\s+m2t_grad_norm_workspace_bytes\s*\(\s*void\s*\)", hdr)
    assert re.search(r"\bint\s+m2t_adam_step_ex\s*\(\s*float\*\s*params,\s*const float\*\s*grads,\s*float\*\s*exp_avg,"
                     r"\s*float\*\s*exp_avg_sq,\s*long long n,\s*float lr,\s*float beta1,\s*float beta2,\s*float eps,\s*int step,"
                     r"\s*float grad_scale,\s*float\*\s*ema,\s*float weight_decay,\s*int decoupled,\s*float ema_decay,"
                     r"\s*const double\*\s*record,\s*void\*\s*stream\)", hdr)
    # each declaration cites the reference's optimizer lines and the torch calls it restates
    for name, calls in (("m2t_grad_norm", ("clip_grad_norm_",)), ("m2t_adam_step_ex", ("torch.optim.Adam", "clip_grad_norm_"))):
        comment = hdr[:hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "train.py:81,210" in comment and all(c in comment for c in calls), name
    lib = _lib.load()
    for name in ("m2t_grad_norm", "m2t_grad_norm_workspace_bytes", "m2t_adam_step_ex"):
        assert hasattr(lib, name)
    ws = lib.m2t_grad_norm_workspace_bytes()
    assert ws > 0 and ws % 8 == 0
    # the argument errors are decided on the host, before anything touches a device (the non-null pointers are never used)
    x = C.c_void_p(0x1000)
    bad_norm = [(None, 4, 1.0, 1.0, 0, 1, 0.9, 0.999, x, x, None),        # null grads with n > 0
                (x, -1, 1.0, 1.0, 0, 1, 0.9, 0.999, x, x, None),          # n < 0
                (x, 4, 1.0, 1.0, 0, 1, 0.9, 0.999, None, x, None),        # no record
                (x, 4, 1.0, 1.0, 0, 1, 0.9, 0.999, x, None, None),        # no workspace
                (x, 4, 1.0, 1.0, 0, 0, 0.9, 0.999, x, x, None)]           # step < 1
    for a in bad_norm:
        assert lib.m2t_grad_norm(*a) != 0, a
        assert b"m2t_grad_norm" in lib.m2t_last_error_string()
    ok = dict(p=x, g=x, m=x, v=x, n=4, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, step=1, gs=1.0, ema=None, wd=0.0, dec=0, d=0.0, rec=None)
    bad_step = [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=-1), dict(step=0), dict(wd=-1e-3), dict(d=1.0),
                dict(d=-0.1), dict(d=float("nan")), dict(wd=float("nan"))]
    for change in bad_step:
        a = dict(ok, **change)
        assert lib.m2t_adam_step_ex(a["p"], a["g"], a["m"], a["v"], a["n"], a["lr"], a["b1"], a["b2"], a["eps"], a["step"],
                                    a["gs"], a["ema"], a["wd"], a["dec"], a["d"], a["rec"], None) != 0, change
        assert b"m2t_adam_step_ex" in lib.m2t_last_error_string()
    # n = 0 is not an error and launches nothing
    assert lib.m2t_adam_step_ex(None, None, None, None, 0, 1e-4, 0.9, 0.999, 1e-8, 1, 1.0, None, 0.0, 0, 0.0, None, None) == 0


def test_train_step_rejects_bad_option_values_before_touching_a_device():
    from m2trans_amd import _lib
    from m2trans_amd.train_step import TrainStep
    ts = TrainStep.__new__(TrainStep)
    ts.model = types.SimpleNamespace(flat_params=torch.zeros(8))
    for kw in (dict(max_grad_norm=0.0), dict(max_grad_norm=float("inf")), dict(weight_decay=-1.0), dict(ema_decay=1.0),
               dict(ema_decay=-0.5)):
        with pytest.raises(_lib.M2TError):
            ts._init_optim_options(**dict(DEFAULTS, **kw))
    # every option off: no record, no workspace, no EMA buffer, and the step stays the plain m2t_adam_step call
    ts._init_optim_options(**DEFAULTS)
    assert ts.optim_record is None and ts._norm_ws is None and ts.ema_params is None and ts._optim_ex is False
    assert ts.grad_norm is None and ts.clip_coef is None and ts.skipped_steps is None
    ts.step_count = 3
    assert ts.applied_step_count() == 3
    with pytest.raises(_lib.M2TError, match="ema_decay=None"):
        ts.swap_ema()


# ------------------------------------------------------------------------------------------------ the yardstick against torch
N_ELEMS = 3_629_760
OPTION_SETS = [("none", None, 0.0, False), ("clip", 100.0, 0.0, False), ("clip_coupled", 100.0, 1e-2, False),
               ("clip_decoupled", 100.0, 1e-2, True)]


def _inputs(step: int, n: int = N_ELEMS):
    """Gradient magnitudes spread over six decades (1e-6 .. 1), random signs; step 3 carries a x50 spike."""
    g = np.random.default_rng(100 + step)
    mag = 10.0 ** g.uniform(-6.0, 0.0, n)
    out = (mag * g.choice([-1.0, 1.0], n)).astype(np.float32)
    return out * np.float32(50.0) if step == 3 else out


@pytest.mark.parametrize("name,max_norm,wd,decoupled", OPTION_SETS, ids=[o[0] for o in OPTION_SETS])
def test_restatement_against_torch_adam(name, max_norm, wd, decoupled):
    """6 teacher-forced steps (both arms start every step from torch's state; torch gets the SAME clipped gradient fp32(g c) and
    the hyper-parameters as the fp32 values the C ABI carries) of torch.optim.Adam(weight_decay, decoupled_weight_decay,
    foreach=False) against step_f32, with step_f64 as the scale.

    Bounds, from counting roundings (each at most 2^-24 of its result; U_m, U_v, G as in tests/optim_ref.py):
      m: torch's lerp (g - m, * w, + m: 3 roundings, its terms up to 1 + w = 1.11 times ours) + ours (b1 m, (1-b1) g', +: 3) +
         the fp32 weights of either arm (2) and, with coupled decay, g' = g c + wd p in either arm (2 + 2 roundings of G
         through 1-b1)                                                            ->  9 U_m (13 U_m coupled)
      v: torch's mul_ + addcmul_ (4) + ours (4), coupled: g'^2 moves by 2 |g'| dg <= 2 G dg, dg = 4 2^-24 G  ->  8 U_v (16 coupled)
      p: 2 ulp(p) for the decay product and the final subtraction of either arm, + what m and v hand on through
         u = (lr/bc1) m / (sqrt(v)/sqrt(bc2) + eps): (lr/bc1)/denom dm + |u| (1/2) dv / v, + 16 roundings of u itself
         (sqrt, two divisions, + eps, the product, the two bias terms and the step size, in either arm).
    Elements where coupled decay cancels (|g'| < 2^-10 G) are left out of the p gate; their share is capped at 1e-3.
    Printed per step: the restatement's own figures against fp64 (p beyond 2 ulp in units of lr, m and v in their units)."""
    h = R.hyper32(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, wd=wd)
    coupled = wd != 0 and not decoupled
    rng = np.random.default_rng(7)
    p0 = (rng.standard_normal(N_ELEMS) * 0.05).astype(np.float32)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"],
                           decoupled_weight_decay=decoupled, foreach=False)
    m0 = np.zeros(N_ELEMS, np.float32)
    v0 = np.zeros(N_ELEMS, np.float32)
    k_m, k_v = (13.0, 16.0) if coupled else (9.0, 8.0)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0, "left_out": 0.0}
    for step in range(1, 7):
        g = _inputs(step)
        coef = R.clip_coef(R.norm64(g), max_norm)
        assert (coef < 1.0) == (max_norm is not None)
        gc = g * np.float32(coef)
        kw = dict(lr=h["lr"], b1=h["b1"], b2=h["b2"], eps=h["eps"], t=step, wd=h["wd"], decoupled=decoupled)
        r32 = R.step_f32(p0, gc, m0, v0, **kw)
        r64 = R.step_f64(p0, gc, m0, v0, **kw)
        tp.grad = torch.from_numpy(gc.copy())
        opt.step()
        st = opt.state[tp]
        assert int(st["step"]) == step
        tp_, tm, tv = tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        # the restatement against fp64: the orientation figures
        d64 = R.deviations(r32, r64)
        keep = ~R.cancelled(r64)
        left_out = 1.0 - keep.mean()
        print(f"{name} step {step}: coef {coef:.4g}; vs fp64: p beyond 2 ulp {d64['p_beyond'][keep].max() / h['lr']:.3g} lr, "
              f"m {d64['m'].max():.2f} U_m, v {d64['v'].max():.2f} U_v; cancelled share {left_out:.2e}")
        assert left_out <= R.CANCEL_CAP, left_out
        # the restatement against torch
        u_m, u_v = R.EPS24 * r64["s_m"] + 2.0 ** -149, R.EPS24 * r64["s_v"] + 2.0 ** -149
        dm = np.abs(r32[1].astype(np.float64) - tm) / u_m
        dv = np.abs(r32[2].astype(np.float64) - tv) / u_v
        bound_p = (2.0 * R.ulp32(r64["p"]) + r64["lr_over_bc1"] / r64["denom"] * k_m * u_m
                   + np.abs(r64["u"]) * (16.0 * R.EPS24 + 0.5 * k_v * u_v / np.maximum(r64["v"], 2.0 ** -126)))
        dp = np.abs(r32[0].astype(np.float64) - tp_) / bound_p
        print(f"    vs torch: m {dm.max():.2f} U_m (gate {k_m}), v {dv.max():.2f} U_v (gate {k_v}), "
              f"p {dp[keep].max():.3f} of its bound, {np.abs(r32[0].astype(np.float64) - tp_)[keep].max() / h['lr']:.3g} lr")
        worst = {"m": max(worst["m"], dm.max()), "v": max(worst["v"], dv.max()), "p": max(worst["p"], dp[keep].max()),
                 "left_out": max(worst["left_out"], left_out)}
        # teacher forcing: the next step of both arms starts from torch's state
        p0, m0, v0 = tp_.copy(), tm.copy(), tv.copy()
    assert worst["m"] <= k_m and worst["v"] <= k_v and worst["p"] <= 1.0, worst


def test_restatement_details_ema_skip_of_nothing_and_the_coefficient():
    """The pieces the torch arm does not cover: EMA against its fp64 form (3 roundings: <= 3 U_e beyond what p hands on), the
    coefficient formula at its edges, bias terms, and that the restatement leaves its inputs alone."""
    rng = np.random.default_rng(3)
    n = 4099
    p, g = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 1e-2).astype(np.float32)
    m, v = (rng.standard_normal(n) * 1e-3).astype(np.float32), (rng.random(n) * 1e-5).astype(np.float32)
    e = (p + rng.standard_normal(n).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    keep = [a.copy() for a in (p, g, m, v, e)]
    kw = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, t=5, coef=0.25, wd=1e-2, decoupled=True, ema_decay=0.999)
    r32, r64 = R.step_f32(p, g, m, v, e, **kw), R.step_f64(p, g, m, v, e, **kw)
    assert all(np.array_equal(a, b) for a, b in zip((p, g, m, v, e), keep))
    d = R.deviations(r32, r64)
    assert d["m"].max() <= 3.5 and d["v"].max() <= 4.5, (d["m"].max(), d["v"].max())
    # ema = d ema + (1-d) p: two products and a sum, + p's own distance from fp64 through (1-d)
    e_bound = 3.0 + (1.0 - 0.999) * d["p_abs"] / (R.EPS24 * r64["s_e"])
    assert (d["ema"] <= e_bound).all(), float((d["ema"] / e_bound).max())
    # ema_decay = 0: the EMA is the weights, bit for bit
    assert np.array_equal(R.step_f32(p, g, m, v, e, **dict(kw, ema_decay=0.0))[3], R.step_f32(p, g, m, v, **kw)[0])
    # coef = 1, no decay: the plain Adam formula
    plain = R.step_f32(p, g, np.zeros_like(p), np.zeros_like(p), lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, t=1)      # (torch's first step)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g.copy())
    h = R.hyper32(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8)
    torch.optim.Adam([tp], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], foreach=False).step()
    assert np.abs(plain[0].astype(np.float64) - tp.detach().numpy()).max() <= 2.0 * np.spacing(np.abs(p)).max()
    assert R.clip_coef(10.0, None) == 1.0 and R.clip_coef(10.0, 0.0) == 1.0 and R.clip_coef(0.5, 1.0) == 1.0
    assert R.clip_coef(4.0, 1.0) == float(np.float32(1.0) / (np.float32(4.0) + np.float32(1e-6)))
    assert R.clip_coef(float("inf"), 1.0) == 0.0 and np.isnan(R.clip_coef(float("nan"), 1.0))
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    assert R.bias_terms(0.9, 0.999, 3) == (1.0 - b1 ** 3, (1.0 - b2 ** 3) ** 0.5)
    x = np.array([3.0, -4.0], np.float32)
    assert R.norm64(x) == 5.0 and R.norm64(x, 0.5) == 2.5


# ------------------------------------------------------------------------------------------------------------- checkpoint
def _model(nb=1):
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=nb, colors=3))


class _Step:
    """The flat-buffer part of TrainStep on the CPU (as tests/test_host_cpu.py's _FakeStep), with the optimizer options."""

    def __init__(self, m, step_count=7, lr=5e-5, skipped=0, **opts):
        g = torch.Generator().manual_seed(step_count)
        self.exp_avg = torch.randn(m.flat_params.shape, generator=g)
        self.exp_avg_sq = torch.rand(m.flat_params.shape, generator=g)
        self.step_count, self.lr, self.betas, self.eps = step_count, lr, (0.9, 0.999), 1e-8
        self.scheduler_last_epoch = 0
        for k, v in dict(DEFAULTS, **opts).items():
            setattr(self, k, v)
        self.optim_record = self.skipped_steps = self.ema_params = None
        if self.max_grad_norm is not None or self.skip_nonfinite or self.track_grad_norm:
            self.optim_record = torch.zeros(8, dtype=torch.float64)
            self.optim_record[4] = skipped
            self.skipped_steps = self.optim_record[4]
        if self.ema_decay is not None:
            self.ema_params = m.flat_params.detach().clone() + 0.01 * torch.randn(m.flat_params.shape, generator=g)

    def set_lr(self, lr):
        self.lr = lr


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    return type(a) is type(b) and a == b


def test_checkpoint_with_every_option_off_is_todays_dict():
    from m2trans_amd.checkpoint import export_checkpoint
    m = _model()
    bare = types.SimpleNamespace(lr=5e-5, step_count=7, exp_avg=torch.randn_like(m.flat_params),
                                 exp_avg_sq=torch.rand_like(m.flat_params))                 # an object without any option
    off = _Step(m)
    off.exp_avg, off.exp_avg_sq = bare.exp_avg, bare.exp_avg_sq
    a, b = export_checkpoint(m, bare, epoch=3), export_checkpoint(m, off, epoch=3)
    assert list(a) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict"]
    assert _same(a, b)
    pg = a["optimizer_state_dict"]["param_groups"][0]
    assert pg["weight_decay"] == 0 and pg.get("decoupled_weight_decay", False) is False
    assert float(a["optimizer_state_dict"]["state"][4]["step"]) == 7.0
    # tracking alone changes nothing in the file either
    assert list(export_checkpoint(m, _Step(m, track_grad_norm=True), epoch=3)) == list(a)


@pytest.mark.parametrize("decoupled", [False, True])
def test_checkpoint_with_options_round_trips_and_feeds_a_stock_adam(decoupled):
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model()
    src = _Step(m, step_count=7, skipped=2, max_grad_norm=0.5, weight_decay=1e-2, decoupled_weight_decay=decoupled,
                ema_decay=0.999, skip_nonfinite=True)
    ck = export_checkpoint(m, src, epoch=3)
    assert list(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict",
                        "ema_state_dict", "m2t_optim"]
    assert ck["m2t_optim"] == {"max_grad_norm": 0.5, "ema_decay": 0.999, "skip_nonfinite": True, "skipped_steps": 2}
    osd = ck["optimizer_state_dict"]
    assert osd["param_groups"][0]["weight_decay"] == 1e-2 and osd["param_groups"][0]["decoupled_weight_decay"] is decoupled
    steps = {float(s["step"]) for s in osd["state"].values()}
    assert steps == {5.0}, steps                                   # the APPLIED step number: 7 calls, 2 skipped
    # a stock torch Adam accepts the optimizer state (train.py:101)
    stock = torch.optim.Adam(list(m.parameters()), lr=1e-4, weight_decay=1e-2, decoupled_weight_decay=decoupled)
    stock.load_state_dict(osd)
    assert stock.param_groups[0]["weight_decay"] == 1e-2 and len(stock.state) == len(m._names)
    # the EMA entry: the model's own names behind "module." (11 + 14 per block: 123 for the 8-block model), loadable strictly
    sd = m.state_dict()
    assert list(ck["ema_state_dict"]) == ["module." + k for k in sd] and len(sd) == 11 + 14 * 1 == len(m._names) + 4
    m2 = _model()
    m2.load_state_dict({k[len("module."):]: v for k, v in ck["ema_state_dict"].items()}, strict=True)
    assert torch.equal(m2.flat_params, src.ema_params)
    # into a step object built with other options (and a stale skipped count): everything comes from the file
    m3 = _model()
    dst = _Step(m3, step_count=99, skipped=5, max_grad_norm=3.0, skip_nonfinite=False, ema_decay=0.5)
    assert import_checkpoint(ck, m3, dst) == 4
    assert (dst.max_grad_norm, dst.weight_decay, dst.decoupled_weight_decay, dst.ema_decay, dst.skip_nonfinite) == \
           (0.5, 1e-2, decoupled, 0.999, True)
    assert dst.step_count == 5 and float(dst.optim_record[4]) == 0.0 and dst.lr == 5e-5
    assert torch.equal(dst.ema_params, src.ema_params) and torch.equal(dst.exp_avg, src.exp_avg)
    assert torch.equal(m3.flat_params, m.flat_params)
    # a file without the EMA entry re-seeds the EMA from the loaded weights
    ck2 = {k: v for k, v in ck.items() if k != "ema_state_dict"}
    dst2 = _Step(_model(), ema_decay=0.999, max_grad_norm=0.5)
    m4 = _model()
    import_checkpoint(ck2, m4, dst2)
    assert torch.equal(dst2.ema_params, m4.flat_params) and torch.equal(m4.flat_params, m.flat_params)


def test_ema_state_dict_helper_uses_the_models_names():
    from m2trans_amd.checkpoint import ema_state_dict
    m = _model()
    ema = torch.arange(m.flat_params.numel(), dtype=torch.float32)
    sd = ema_state_dict(m, ema)
    ref = m.state_dict()
    assert list(sd) == list(ref)
    frozen = [k for k in ref if k not in m._names]
    assert len(frozen) == 4 and all(torch.equal(sd[k], ref[k]) for k in frozen)
    for n, (o, k, shp) in zip(m._names, m._slots):
        assert sd[n].shape == torch.Size(shp) and torch.equal(sd[n].reshape(-1), ema[o:o + k])
    before = ema.clone()
    for n in m._names:
        sd[n].add_(1.0)                                            # copies, not views
    assert torch.equal(ema, before)


# ------------------------------------------------------------------------------------------------------------ timing tool
def test_timing_tool_host_part_runs_without_a_device():
    """tools/optim_timing.py: argument parsing, configs[1]'s shapes, the byte model and the keys of the JSON line."""
    spec = importlib.util.spec_from_file_location("optim_timing", os.path.join(ROOT, "tools", "optim_timing.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    args = T.parse_args([])
    assert (args.batch, args.lr_size, args.dtype, args.blocks) == (16, 128, "bf16", 8) and args.repeats >= 5
    assert T.shapes(args) == ((16, 3, 128, 128), (16, 3, 512, 512))
    assert T.options(args) == {"max_grad_norm": 1.0, "weight_decay": 1e-2, "decoupled_weight_decay": True, "ema_decay": 0.999,
                               "skip_nonfinite": True}
    with pytest.raises(SystemExit):
        T.parse_args(["--repeats", "4"])
    n = 3_629_760
    assert T.traffic(n) == (7, 10, 3 * 4 * n) and T.traffic(n, ema=False) == (7, 8, 4 * n)
    out = T.result(args, [4.50, 4.52, 4.48, 4.50, 4.51], [4.52, 4.53, 4.51, 4.52, 4.52], n)
    assert tuple(out) == T.RESULT_KEYS
    assert out["overhead_ms"] == 0.02 and out["plain_spread"] == round(0.04 / 4.50, 4)
    assert out["overhead_within_plain_spread"] is True and out["overhead_within_1_percent"] is True
    slow = T.result(args, [4.50] * 5, [4.60] * 5, n)
    assert slow["overhead_within_plain_spread"] is False and slow["overhead_within_1_percent"] is False
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="needs a HIP device"):
            T.main([])
