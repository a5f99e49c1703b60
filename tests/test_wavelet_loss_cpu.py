"""CPU tests (no GPU) of the wavelet-domain loss term (TrainStep(lambda_wavelet=...), m2t_wavelet_loss / m2t_wavelet_loss_tensor /
m2t_swt2): the fp64 restatement the GPU tests compare the kernels with (tests/wavelet_loss_ref.py) -- Parseval for the two built-in
filters, the inner-product identity of its adjoint, its closed-form gradient against torch autograd where autograd is smooth and
against a finite difference where it is not --, the C ABI table of include/m2t_wavelet.h, the refusals of the C entries and of
resolve_wavelet, TrainStep's call sequence, the meter columns, the checkpoint entry, and the kernel text run on host threads
(tests/wavelet_emulate.cpp) under the gate of the GPU test, once more under ASan / UBSan."""
import contextlib
import ctypes as C
import inspect
import os
import re
import shutil
import struct
import subprocess
import types

import pytest
import torch

from tests import wavelet_loss_ref as Wv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_ULP = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["haar", "db2"])
@pytest.mark.parametrize("hw", [(13, 14), (33, 70)], ids=["13x14", "33x70"])
def test_the_built_in_filters_give_a_tight_frame(name, hw):
    """sum_bands ||c||^2 = ||d||^2 to 1e-12 relative, at 3 levels (13 is the smallest side db2 takes there)."""
    lo, hi = Wv.FILTERS[name]
    assert abs(sum(lo) - 1.0) < 1e-15 and abs(sum(hi)) < 1e-15 and hi == tuple((-1.0) ** k * lo[len(lo) - 1 - k] for k in range(len(lo)))
    d = torch.randn((2, 3) + hw, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for J in (1, 2, 3):
        bands = Wv.swt2(d, lo, hi, J)
        assert len(bands) == 3 * J + 1 and all(b.shape == d.shape for b in bands)
        e, ref = sum(float((b * b).sum()) for b in bands), float((d * d).sum())
        assert abs(e - ref) <= 1e-12 * ref, (J, e, ref)


@pytest.mark.parametrize("name", ["haar", "db2", "tri"])
def test_the_adjoint_satisfies_the_inner_product_identity(name):
    """<W d, psi> = <d, W^T psi>, the non-orthogonal 3-tap pair included; absent bands add nothing."""
    lo, hi = Wv.FILTERS[name]
    g = torch.Generator().manual_seed(2)
    for hw, J in (((13, 14), 3), ((33, 70), 2), ((7, 5), 1)):
        d = torch.randn((1, 2) + hw, generator=g, dtype=torch.float64)
        psi = [torch.randn(d.shape, generator=g, dtype=torch.float64) for _ in range(3 * J + 1)]
        psi[1] = None
        if J > 1:
            psi[3 * J] = None
        lhs = sum(float((c * p).sum()) for c, p in zip(Wv.swt2(d, lo, hi, J), psi) if p is not None)
        rhs = float((d * Wv.adjoint(psi, lo, hi, J)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (name, hw, J, lhs, rhs)


def _roll_swt_value(x, y, R, clamp, lo, hi, J, weights, eps):
    """The term through torch ops autograd can follow (an fp64 SWT built from torch.roll, written independently of the restatement)."""
    d = ((x.clamp(0.0, R) if clamp else x) - y) / R
    total, a = 0.0, d
    for j in range(J):
        s = 2 ** j
        row = lambda t, f: sum(f[k] * torch.roll(t, -k * s, dims=3) for k in range(len(f)))
        col = lambda t, f: sum(f[k] * torch.roll(t, -k * s, dims=2) for k in range(len(f)))
        rl, rh = row(a, lo), row(a, hi)
        for b, c in enumerate((col(rl, hi), col(rh, lo), col(rh, hi))):
            total = total + weights[3 * j + b] * torch.sqrt(c * c + eps * eps).sum()
        a = col(rl, lo)
    total = total + weights[3 * J] * torch.sqrt(a * a + eps * eps).sum()
    return total / x.numel()


@pytest.mark.parametrize("name,J,shape,R,clamp", [("haar", 3, (2, 3, 13, 14), 1.0, True), ("db2", 3, (2, 3, 33, 70), 255.0, True),
                                                 ("tri", 2, (1, 1, 20, 9), 1.0, False)])
def test_the_closed_form_gradient_equals_autograd_where_autograd_is_smooth(name, J, shape, R, clamp):
    """eps = 1e-3: the closed form against autograd through a roll-built SWT, 1e-10 relative to the largest element; LL weighted."""
    lo, hi = Wv.FILTERS[name]
    weights = [1.0 + 0.25 * b for b in range(3 * J)] + [0.5]
    x, y = Wv.mixed_pair(shape, seed=3, R=R)
    val, grad, sums, _ = Wv.value_and_grad(x, y, R, clamp, None, lo, hi, J, weights, 1e-3)
    leaf = x.double().requires_grad_(True)
    v = _roll_swt_value(leaf, y.double(), R, clamp, lo, hi, J, weights, 1e-3)
    v.backward()
    top = float(leaf.grad.abs().max())
    assert top > 0 and abs(val - float(v.detach())) <= 1e-12 * abs(float(v.detach()))
    assert float((grad - leaf.grad).abs().max()) <= 1e-10 * top
    if clamp:
        assert int(torch.count_nonzero(grad[(x < 0) | (x > R)])) == 0 and int(((x < 0) | (x > R)).sum()) > 0


def test_the_l1_gradient_equals_a_central_difference_away_from_the_sector():
    """eps = 0: |c| is linear around every gated coefficient (smallest non-zero |c| >= 1e-7 here, asserted), so a central difference
    with h = 1e-8 -- which moves a coefficient by at most 1.19^4 h -- crosses no kink and is exact up to rounding; 20 elements away
    from the sector.  The difference of the two values is taken coefficient by coefficient, sum(|c+| - |c-|), so that the total
    (about 2e3) does not cancel: each difference carries 2 ulp(|c|) = 2e-17, over 2 h that is 1e-9, times at most 6 bands x 49
    coefficients in reach: 3e-7, gated at 1e-6."""
    shape, J = (1, 3, 33, 70), 2
    lo, hi = Wv.DB2
    x, y = Wv.mixed_pair(shape, seed=4)
    x, y = x.double(), y.double()
    val, grad, sums, smallest = Wv.value_and_grad(x, y, 1.0, False, 1.0, lo, hi, J)
    assert smallest >= 1e-7
    h = 1e-8
    g = torch.Generator().manual_seed(5)
    n = 0
    while n < 20:
        ch, r, c = int(torch.randint(3, (1,), generator=g)), int(torch.randint(33, (1,), generator=g)), int(torch.randint(70, (1,), generator=g))
        if r < 11 + 12 and c < 23 + 12:                        # inside or within the cascade's reach of the sector
            continue
        xp, xm = x.clone(), x.clone()
        xp[0, ch, r, c] += h
        xm[0, ch, r, c] -= h
        bp, bm = Wv.swt2(Wv.difference(xp, y, 1.0, False), lo, hi, J), Wv.swt2(Wv.difference(xm, y, 1.0, False), lo, hi, J)
        fd = sum(float((p.abs() - m.abs()).sum()) for p, m in zip(bp[:3 * J], bm[:3 * J])) / (2 * h)
        assert abs(fd - float(grad[0, ch, r, c])) <= 1e-6, (ch, r, c, fd, float(grad[0, ch, r, c]))
        n += 1


def test_the_sector_has_exactly_zero_coefficients_and_gradient_and_a_zero_weight_equals_leaving_the_band_out():
    shape, J = (1, 3, 70, 33), 3
    lo, hi = Wv.HAAR
    x, y = Wv.mixed_pair(shape, seed=6, div=2)
    sec = Wv.sector(shape, 2, J, div=2)
    assert int(sec.sum()) > 0
    val, grad, sums, smallest = Wv.value_and_grad(x, y, 1.0, True, None, lo, hi, J)
    assert int(torch.count_nonzero(grad[sec])) == 0 and float(grad.abs().max()) > 0 and smallest >= 1e-7
    w = Wv.default_weights(J)
    w[1], w[5] = 0.0, 0.0
    full = [1.0] * (3 * J) + [0.0]
    a = Wv.value_and_grad(x, y, 1.0, True, None, lo, hi, J, w)
    b = Wv.value_and_grad(x, y, 1.0, True, None, lo, hi, J, full, skip=(1, 5))
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and a[0] < val


# ------------------------------------------------------------------------------------------------------------- C ABI
def _arr(v):
    return (C.c_double * len(v))(*v)


def test_entry_points_decide_sizes_and_bad_arguments_on_the_host():
    from m2trans_amd import _lib
    lib = _lib.load()
    sb = lib.m2t_wavelet_loss_scratch_bytes
    # levels, taps, channels, batch, the smallest side
    for bad in ((1, 3, 64, 64, 0, 2), (1, 3, 64, 64, 4, 2), (1, 3, 64, 64, 2, 1), (1, 3, 64, 64, 2, 9), (1, 2, 64, 64, 2, 2),
                (0, 3, 64, 64, 2, 2), (21846, 3, 64, 64, 1, 2), (65536, 1, 64, 64, 1, 2), (1, 3, 1, 64, 1, 2), (1, 3, 64, 12, 3, 4),
                (1, 3, 12, 64, 3, 4), (1, 3, 28, 64, 3, 8)):
        assert sb(*bad) == 0, bad
    assert _lib.wavelet_min_side(4, 3) == 13 and _lib.wavelet_min_side(2, 1) == 2 and _lib.wavelet_min_side(8, 3) == 29
    # (3 J + 3) planes of doubles and 3 J + 1 sums per 32 x 32 tile of every (image, channel)
    assert sb(1, 1, 2, 2, 1, 2) == 8 * (6 * 4 + 4 * 1)
    assert sb(2, 3, 13, 14, 3, 4) == 8 * (12 * 6 * 13 * 14 + 10 * 6)
    assert sb(2, 3, 33, 70, 3, 4) == 8 * (12 * 6 * 33 * 70 + 10 * 6 * 2 * 3)
    assert sb(21845, 3, 64, 64, 2, 2) == 8 * (9 * 65535 * 4096 + 7 * 65535 * 4)
    one = C.c_void_p(8)                                              # a non-null pointer that is never followed
    lo, hi, w7 = _arr(Wv.DB2[0]), _arr(Wv.DB2[1]), _arr([1.0] * 6 + [0.0])
    call = lambda **kw: lib.m2t_wavelet_loss_tensor(*[kw.get(k, v) for k, v in (
        ("x", one), ("y", one), ("B", 1), ("C", 3), ("H", 48), ("W", 64), ("xs", 3 * 48 * 64), ("rs", 64), ("dr", 1.0), ("clamp", 1),
        ("scale", 1.0), ("lo", lo), ("hi", hi), ("taps", 4), ("levels", 2), ("bw", w7), ("eps", 0.0), ("gx", None), ("loss", one),
        ("per", None), ("acc", 0), ("scratch", one), ("stream", None))])
    nan, inf = float("nan"), float("inf")
    for bad in (dict(x=None), dict(y=None), dict(lo=None), dict(hi=None), dict(loss=None), dict(scratch=None), dict(H=6), dict(W=6), dict(H=0),
                dict(W=-3), dict(dr=0.0), dict(dr=-1.0), dict(dr=nan), dict(dr=inf), dict(scale=nan), dict(scale=inf), dict(rs=63),
                dict(xs=3 * 48 * 64 - 3), dict(xs=3 * 48 * 64 + 1), dict(B=0), dict(B=-1), dict(B=21846), dict(C=0), dict(C=2, xs=2 * 48 * 64),
                dict(taps=1), dict(taps=9), dict(levels=0), dict(levels=4), dict(eps=-1e-3), dict(eps=nan), dict(eps=inf),
                dict(lo=_arr([0.5, nan, 0.5, 0.0])), dict(hi=_arr([0.5, inf, 0.5, 0.0])), dict(bw=_arr([0.0] * 7)),
                dict(bw=_arr([1.0, -1.0, 1, 1, 1, 1, 0])), dict(bw=_arr([1.0, nan, 1, 1, 1, 1, 0]))):
        assert call(**bad) == -2, bad
    text = lambda **kw: (call(**kw), lib.m2t_last_error_string())[1]
    assert b"wraps at most once" in text(H=6) and b"1 or 3" in text(C=2, xs=2 * 48 * 64) and b"65535" in text(B=21846)
    assert b"levels must be" in text(levels=4) and b"2 to 8 taps" in text(taps=9) and b"taps must be finite" in text(lo=_arr([nan] * 4))
    assert b"not all be 0" in text(bw=_arr([0.0] * 7)) and b"finite and >= 0" in text(bw=_arr([1.0, -1.0, 1, 1, 1, 1, 0]))
    assert b"eps must be" in text(eps=-1.0) and b"null argument" in text(lo=None) and b"m2t_wavelet_loss_tensor" in text(lo=None)
    # the transform alone and the plan entry
    swt = lambda **kw: lib.m2t_swt2(*[kw.get(k, v) for k, v in (
        ("x", one), ("B", 1), ("C", 3), ("H", 48), ("W", 64), ("xs", 3 * 48 * 64), ("rs", 64), ("lo", lo), ("hi", hi), ("taps", 4),
        ("levels", 3), ("out", one), ("scratch", one), ("stream", None))])
    for bad in (dict(x=None), dict(lo=None), dict(hi=None), dict(out=None), dict(scratch=None), dict(H=12), dict(W=12), dict(levels=4),
                dict(taps=0), dict(C=4, xs=4 * 48 * 64), dict(rs=60), dict(B=0), dict(lo=_arr([nan] * 4))):
        assert swt(**bad) == -2, bad
    assert swt(H=12) == -2 and b"m2t_swt2" in lib.m2t_last_error_string() and b"wraps at most once" in lib.m2t_last_error_string()
    assert lib.m2t_wavelet_loss(None, None, 1.0, 1.0, 1.0, None, None, 2, 2, None, 0.0, None, 0, None, None, None) == -2
    assert b"m2t_wavelet_loss" in lib.m2t_last_error_string() and b"null argument" in lib.m2t_last_error_string()


def test_python_entries_refuse_host_tensors_and_bad_arguments():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import WaveletLoss, swt2, wavelet_loss
    x = torch.zeros(1, 3, 8, 8)
    for fn in (wavelet_loss, WaveletLoss()):
        with pytest.raises(M2TError, match="device"):
            fn(x, x)                                                 # host tensors: no fallback
        with pytest.raises(M2TError):
            fn(x, x[..., :6])
    with pytest.raises(M2TError, match="device"):
        swt2(x)
    fake = types.SimpleNamespace(dim=lambda: 4, shape=torch.Size((1, 3, 8, 8)), is_cuda=True, requires_grad=False)
    for kw in (dict(data_range=0.0), dict(data_range=float("nan")), dict(data_range=float("inf"))):
        with pytest.raises(M2TError, match="finite number > 0"):
            wavelet_loss(fake, fake, **kw)
    two = types.SimpleNamespace(dim=lambda: 4, shape=torch.Size((1, 2, 8, 8)), is_cuda=True, requires_grad=False)
    with pytest.raises(M2TError, match="1 or 3 channels"):
        wavelet_loss(two, two)
    with pytest.raises(M2TError, match="at least 13"):
        wavelet_loss(fake, fake, wavelet="db2", levels=3)
    with pytest.raises(M2TError, match="at least 13"):
        swt2(fake, "db2", 3)
    with pytest.raises(M2TError, match="wavelet must be one of"):
        wavelet_loss(fake, fake, wavelet="sym4")
    with pytest.raises(M2TError, match="wavelet_levels"):
        swt2(fake, "haar", 4)
    needs = types.SimpleNamespace(dim=lambda: 4, shape=torch.Size((1, 3, 8, 8)), is_cuda=True, requires_grad=True)
    with pytest.raises(M2TError, match="x only"):
        wavelet_loss(fake, needs)
    m = WaveletLoss(255.0, "DB2", 3, [1.0] * 9 + [0.5], 1e-3)
    assert (m.data_range, m.wavelet, m.levels, m.band_weights, m.eps) == (255.0, "db2", 3, (1.0,) * 9 + (0.5,), 1e-3)


# ------------------------------------------------------------------------------------------------------------- TrainStep
def test_resolve_wavelet_names_what_it_refuses():
    from m2trans_amd import train_step as T
    from m2trans_amd._lib import M2TError
    w = T.resolve_wavelet()
    assert w == ("haar", (0.5, 0.5), (0.5, -0.5), 2, None, 0.0)
    w = T.resolve_wavelet("DB2", 3, [1] * 9 + [0.25], "1e-3")
    assert w.wavelet == "db2" and w.lo == Wv.DB2[0] and w.hi == Wv.DB2[1] and w.band_weights == (1.0,) * 9 + (0.25,) and w.eps == 1e-3
    w = T.resolve_wavelet((Wv.TRI[0], list(Wv.TRI[1])), 1)
    assert w.wavelet == ([0.25, 0.5, 0.25], [-0.25, 0.5, -0.25]) and w.lo == Wv.TRI[0] and w.hi == Wv.TRI[1]
    for bad in ("sym4", None, 3, ("haar",), ((0.5, 0.5),), ((0.5, "x"), (0.5, 0.5))):
        with pytest.raises(M2TError, match="wavelet must be one of"):
            T.resolve_wavelet(bad)
    for bad in (((0.5, 0.5), (0.5, 0.5, 0.5)), ((1.0,), (1.0,)), ((0.1,) * 9, (0.1,) * 9), ((0.5, float("nan")), (0.5, 0.5)),
                ((0.5, 0.5), (float("inf"), 0.5))):
        with pytest.raises(M2TError, match="wavelet taps"):
            T.resolve_wavelet(bad)
    for bad in (0, 4, -1, 2.0, "2", None, True):
        with pytest.raises(M2TError, match="wavelet_levels"):
            T.resolve_wavelet("haar", bad)
    for bad in ([1.0] * 6, [1.0] * 8, [0.0] * 7, [1, 1, 1, 1, 1, 1, -0.5], [1, 1, 1, 1, 1, 1, float("nan")], [1, 1, 1, 1, 1, 1, float("inf")],
                "weights", 1.0, [1, 1, 1, 1, 1, 1, "x"]):
        with pytest.raises(M2TError, match="wavelet_band_weights must be 7"):
            T.resolve_wavelet("haar", 2, bad)
    for bad in (-1e-3, float("nan"), float("inf"), None, "tiny"):
        with pytest.raises(M2TError, match="wavelet_eps"):
            T.resolve_wavelet("haar", 2, None, bad)
    lo, hi, taps, J, bw, eps = T.wavelet_call_args(T.resolve_wavelet("db2", 3, [0.5] * 10, 1e-3))
    assert (list(lo), list(hi), taps, J, list(bw), eps) == (list(Wv.DB2[0]), list(Wv.DB2[1]), 4, 3, [0.5] * 10, 1e-3)
    assert T.wavelet_call_args(T.resolve_wavelet())[4] is None


def test_lambda_wavelet_defaults_setter_and_table():
    from m2trans_amd import train_step as T
    from m2trans_amd._lib import M2TError
    p = inspect.signature(T.TrainStep.__init__).parameters
    assert [p[k].default for k in ("lambda_wavelet", "wavelet", "wavelet_levels", "wavelet_band_weights", "wavelet_eps")] == \
        [0.0, "haar", 2, None, 0.0]
    assert T.TrainStep.lambda_wavelet == 0.0 and T.TrainStep.wavelet_loss is None and T.TrainStep.wavelet == "haar"
    assert T.resolve_lambda_wavelet("0.5") == 0.5
    for bad in (-0.1, float("nan"), None):
        with pytest.raises(M2TError, match="lambda_wavelet"):
            T.resolve_lambda_wavelet(bad)
    with pytest.raises(M2TError, match="lambda_wavelet"):
        T.TrainStep(None, lambda_wavelet=-1.0)
    # the row of the one table (its order: tests/test_loss_terms_cpu.py)
    row = T._TERM["wavelet"]
    assert isinstance(row, T.LossTerm) and row in T.LOSS_TERMS
    assert row.size_ok(13, 500, 3, 4) and not row.size_ok(12, 500, 3, 4) and not row.size_ok(500, 12, 3, 4) and row.size_ok(2, 2, 1, 2)
    assert row.count(7, 100, 200) == 7 * 3 * 100 * 200
    assert all(t.shape_args(None) == () for t in T.LOSS_TERMS if t is not row)
    ts = T.TrainStep.__new__(T.TrainStep)
    ts.accum_steps, ts.micro_count = 2, 1
    with pytest.raises(M2TError, match="accumulation cycle"):
        ts.set_lambda_wavelet(0.0)
    ts.micro_count = 0
    ts.set_lambda_wavelet(0.0, "db2", 3)
    assert ts.lambda_wavelet == 0.0 and ts.wavelet_loss is None and ts._wavelet_scratch == {} and (ts.wavelet, ts.wavelet_levels) == ("db2", 3)
    with pytest.raises(M2TError, match="wavelet_band_weights must be 10"):
        ts.set_lambda_wavelet(0.0, band_weights=[1.0] * 7)
    assert ts.wavelet_band_weights is None
    extra = row.extra(ts)
    assert list(extra[0]) == list(Wv.DB2[0]) and extra[2:4] == (4, 3) and extra[4] is None and extra[5] == 0.0 and row.shape_args(ts) == (3, 4)
    # a size the term does not take is refused on the host: no library call is made (lib = None would raise otherwise)
    with pytest.raises(M2TError, match="lambda_wavelet > 0: .*reach of the filters"):
        ts._scratch_for(row, None, torch.zeros(2, 3, 12, 64))


class _Calls:
    """A stand-in for the loaded library: records the entry points in call order, every call succeeds."""

    def __init__(self):
        self.names, self.args = [], {}

    def __getattr__(self, name):
        def fn(*a):
            self.names.append(name)
            self.args[name] = a
            return 1 << 20 if name.endswith("scratch_bytes") or name.endswith("workspace_bytes") else 0
        return fn


def _host_step(monkeypatch, accum=1, **terms):
    """TrainStep.forward_backward on the host against _Calls: the step object assembled without __init__, no device needed."""
    from m2trans_amd import _lib, train_step as T
    calls = _Calls()
    monkeypatch.setattr(_lib, "load", lambda: calls)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(_lib, "ptr", lambda t: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    plan = types.SimpleNamespace(handle=None, workspace=None, gen=0, trained=False)
    model = types.SimpleNamespace(scale=2, rgb_range=1.0, flat_params=torch.zeros(4), _plan_for=lambda lr: plan)
    ts = T.TrainStep.__new__(T.TrainStep)
    ts.model, ts.micro_count, ts.accum_steps, ts.world_size = model, 0, accum, 1
    ts.semantic_loss, ts.lambda_clip, ts.lambda_l1 = None, 0.0, 1.0
    ts.grads, ts.micro_grads, ts.l1_loss, ts.micro_loss = torch.zeros(4), torch.zeros(4), torch.zeros(1), torch.zeros(1)
    ts.set_pixel_loss("l1", None)
    for k, v in terms.items():
        if k == "lambda_perceptual":
            ts.perceptual_loss = types.SimpleNamespace(loaded=True, resize=False, data_range=1.0, handle=None, kind=0, param=0.0,
                                                       tap_weights=lambda: None, workspace=lambda *a: None)
            ts.set_lambda_perceptual(v)
        elif isinstance(v, tuple):
            getattr(ts, "set_" + k)(*v)
        else:
            getattr(ts, "set_" + k)(v)
    ts.forward_backward(torch.zeros(2, 3, 96, 96), torch.zeros(2, 3, 192, 192))
    return ts, calls


def test_lambda_wavelet_zero_issues_todays_call_sequence(monkeypatch):
    today = ["m2t_forward", "m2t_l1_loss_deferred", "m2t_backward"]
    _, bare = _host_step(monkeypatch)
    ts, zero = _host_step(monkeypatch, lambda_wavelet=(0.0, "db2", 3))
    assert bare.names == today and zero.names == today
    assert ts.wavelet_loss is None and ts._wavelet_scratch == {} and ts._wavelet_call is None          # nothing allocated


def test_lambda_wavelet_call_sequence_alone_and_with_the_other_terms(monkeypatch):
    ts, on = _host_step(monkeypatch, lambda_wavelet=(0.05, "db2", 2, None, 1e-3))
    assert on.names == ["m2t_wavelet_loss_scratch_bytes", "m2t_forward", "m2t_l1_loss", "m2t_wavelet_loss", "m2t_backward"]
    assert on.args["m2t_wavelet_loss_scratch_bytes"] == (2, 3, 192, 192, 2, 4)
    a = on.args["m2t_wavelet_loss"]
    assert len(a) == 16 and a[2] == 0.05 and a[3] == 2.0 * 3 * 192 * 192 and a[4] == 1.0         # weight, divisor = B 3 Hs Ws, R
    assert list(a[5]) == list(Wv.DB2[0]) and list(a[6]) == list(Wv.DB2[1]) and a[7:9] == (4, 2) and a[9] is None and a[10] == 1e-3
    assert a[12] == 0                                                                          # store
    assert list(ts._wavelet_scratch) == [(2, 192, 192, 2, 4)] and ts.wavelet_loss is not None
    assert ts.loss is not ts.l1_loss
    ts, both = _host_step(monkeypatch, lambda_vif=0.1, lambda_gmsd=0.05, lambda_wavelet=(0.05, "haar", 3, [1.0] * 9 + [0.5]), lambda_perceptual=0.2)
    order = [n for n in both.names if not n.endswith("scratch_bytes")]
    assert order == ["m2t_forward", "m2t_l1_loss", "m2t_vif_loss", "m2t_gmsd_loss", "m2t_wavelet_loss", "m2t_vgg_loss", "m2t_backward"]
    assert list(both.args["m2t_wavelet_loss"][9]) == [1.0] * 9 + [0.5] and both.args["m2t_wavelet_loss"][7:9] == (2, 3)
    # the second micro-batch of a cycle: the divisor is the global count, the value is added to
    ts, acc = _host_step(monkeypatch, accum=2, lambda_wavelet=0.05)
    assert acc.args["m2t_wavelet_loss"][3] == 4.0 * 3 * 192 * 192 and acc.args["m2t_wavelet_loss"][12] == 0
    ts.forward_backward(torch.zeros(2, 3, 96, 96), torch.zeros(2, 3, 192, 192))
    assert acc.args["m2t_wavelet_loss"][12] == 1 and acc.names.count("m2t_wavelet_loss_scratch_bytes") == 1


def test_meter_columns_and_the_train_keys():
    from m2trans_amd import train as TR
    k = TR.TRAINSTEP_KEYS
    at = k.index("lambda_gmsd")
    assert k[at + 1:at + 6] == ("lambda_wavelet", "wavelet", "wavelet_levels", "wavelet_band_weights", "wavelet_eps")
    off = types.SimpleNamespace(lambda_gmsd=0.1)
    assert TR.meter_columns(off) == ["loss", "pixel", "clip", "gmsd"]
    on = types.SimpleNamespace(lambda_gmsd=0.05, lambda_wavelet=0.1, lambda_perceptual=0.2, loss=1, l1_loss=2, clip_loss=3, gmsd_loss=4,
                               wavelet_loss=5, perceptual_loss_value=6)
    cols = TR.meter_columns(on)
    assert cols == ["loss", "pixel", "clip", "gmsd", "wavelet", "perceptual"]
    assert TR.meter_values(on, cols) == [1, 2, 3, 4, 5, 6]


# ------------------------------------------------------------------------------------------------------------- checkpoint
def _model():
    from m2trans_amd.M2Trans_network import create_model
    return create_model(types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=1, colors=3))


class _Step:
    """The flat-buffer part of TrainStep on the CPU, with the pixel loss and the weights of the optional terms."""

    def __init__(self, m, pixel_loss="l1", pixel_loss_param=None, step_count=7, lr=5e-5, wavelet=("haar", 2, None, 0.0), **lambdas):
        from m2trans_amd.train_step import TrainStep
        g = torch.Generator().manual_seed(step_count)
        self.exp_avg = torch.randn(m.flat_params.shape, generator=g)
        self.exp_avg_sq = torch.rand(m.flat_params.shape, generator=g)
        self.step_count, self.lr, self.scheduler_last_epoch = step_count, lr, 0
        self.micro_count, self.accum_steps, self.fft_norm = 0, 1, "backward"
        TrainStep.set_pixel_loss(self, pixel_loss, pixel_loss_param)
        for n in ("ssim", "msssim", "fft", "vif", "gmsd", "wavelet"):
            setattr(self, f"lambda_{n}", float(lambdas.get(f"lambda_{n}", 0.0)))
        self.wavelet, self.wavelet_levels, self.wavelet_band_weights, self.wavelet_eps = wavelet

    def set_pixel_loss(self, name, param=None):
        from m2trans_amd.train_step import TrainStep
        TrainStep.set_pixel_loss(self, name, param)

    def set_lambda_wavelet(self, value, wavelet=None, levels=None, band_weights=None, eps=None):
        from m2trans_amd.train_step import resolve_lambda_wavelet, resolve_wavelet
        self.lambda_wavelet = resolve_lambda_wavelet(value)
        w = resolve_wavelet(self.wavelet if wavelet is None else wavelet, self.wavelet_levels if levels is None else levels,
                            self.wavelet_band_weights if band_weights is None else band_weights, self.wavelet_eps if eps is None else eps)
        self.wavelet, self.wavelet_levels, self.wavelet_eps = w.wavelet, w.levels, w.eps
        self.wavelet_band_weights = None if w.band_weights is None else list(w.band_weights)

    def set_lr(self, lr):
        self.lr = lr


def test_checkpoint_entry_carries_the_wavelet_keys_after_the_existing_ones_and_round_trips():
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model()
    keys = ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict"]
    assert list(export_checkpoint(m, _Step(m, lambda_wavelet=0.0, wavelet=("db2", 3, None, 1e-3)), epoch=3)) == keys      # off: today's dict
    src = _Step(m, "sl1", 0.25, lambda_wavelet=0.05, wavelet=("db2", 3, [1.0] * 9 + [0.5], 1e-3))
    ck = export_checkpoint(m, src, epoch=3)
    assert list(ck) == keys + ["m2t_loss"]
    assert ck["m2t_loss"] == {"pixel_loss": "smooth_l1", "param": 0.25, "lambda_wavelet": 0.05, "wavelet": "db2", "wavelet_levels": 3,
                              "wavelet_band_weights": [1.0] * 9 + [0.5], "wavelet_eps": 1e-3}
    every = export_checkpoint(m, _Step(m, lambda_wavelet=0.05, lambda_gmsd=0.05, lambda_ssim=0.1, lambda_msssim=0.16, lambda_fft=0.2,
                                       lambda_vif=0.3), epoch=3)["m2t_loss"]
    assert list(every) == ["pixel_loss", "param", "lambda_ssim", "lambda_msssim", "lambda_fft", "fft_norm", "lambda_vif", "lambda_gmsd",
                           "lambda_wavelet", "wavelet", "wavelet_levels", "wavelet_band_weights", "wavelet_eps"]
    assert every["wavelet"] == "haar" and every["wavelet_band_weights"] is None
    # without the term the entry is the one it was
    assert list(export_checkpoint(m, _Step(m, lambda_gmsd=0.05), epoch=3)["m2t_loss"]) == ["pixel_loss", "param", "lambda_gmsd"]
    for start in ((0.0, ("haar", 2, None, 0.0)), (0.7, ("db2", 2, [2.0] * 7, 0.5))):           # whatever the importing step was built with
        dst = _Step(_model(), "mse", None, lambda_wavelet=start[0], wavelet=start[1], step_count=1)
        assert import_checkpoint(ck, _model(), dst) == 4
        assert (dst.lambda_wavelet, dst.wavelet, dst.wavelet_levels, dst.wavelet_band_weights, dst.wavelet_eps) == \
            (0.05, "db2", 3, [1.0] * 9 + [0.5], 1e-3)
        assert (dst.pixel_loss, dst.pixel_loss_param) == ("smooth_l1", 0.25) and dst.step_count == 7 and torch.equal(dst.exp_avg, src.exp_avg)
    # a custom pair travels as its two tap lists; default weights come back as the default
    ck2 = export_checkpoint(m, _Step(m, lambda_wavelet=0.1, wavelet=((list(Wv.TRI[0]), list(Wv.TRI[1])), 1, None, 0.0)), epoch=3)
    assert ck2["m2t_loss"]["wavelet"] == [list(Wv.TRI[0]), list(Wv.TRI[1])]
    dst = _Step(_model(), lambda_wavelet=0.7, wavelet=("db2", 1, [2.0] * 4, 0.5))
    import_checkpoint(ck2, _model(), dst)
    assert dst.wavelet == ([0.25, 0.5, 0.25], [-0.25, 0.5, -0.25]) and dst.wavelet_band_weights is None and dst.wavelet_eps == 0.0
    # a file without the key loads as 0 into a fresh step
    dst = _Step(_model())
    import_checkpoint(export_checkpoint(m, _Step(m, "mse", lambda_vif=0.3), epoch=3), _model(), dst)
    assert dst.lambda_wavelet == 0.0 and dst.pixel_loss == "mse"
    # a plain object without the setters receives the attributes
    plain = types.SimpleNamespace(lr=1.0, step_count=0, exp_avg=torch.zeros_like(m.flat_params), exp_avg_sq=torch.zeros_like(m.flat_params),
                                  scheduler_last_epoch=0, set_lr=lambda lr: None)
    import_checkpoint(ck, _model(), plain)
    assert (plain.lambda_wavelet, plain.wavelet, plain.wavelet_levels, plain.wavelet_eps) == (0.05, "db2", 3, 1e-3)
    assert plain.wavelet_band_weights == [1.0] * 9 + [0.5]


# ------------------------------------------------------------------------------------------------------------- host emulation
def _compiler():
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"), shutil.which("clang++"), shutil.which("g++"))
                if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler found"
    return cxx


def _build_emulator(path, flags):
    subprocess.run([_compiler(), "-x", "c++", "-std=c++20", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "tests", "emulate_hip"),
                    "-I", os.path.join(ROOT, "m2trans_amd", "csrc"), os.path.join(ROOT, "tests", "wavelet_emulate.cpp"), "-o", path,
                    "-lpthread"], check=True, capture_output=True)
    return path


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return _build_emulator(str(tmp_path_factory.mktemp("wavelet") / "wavelet_emulate"), ["-O2"])


@pytest.fixture(scope="module")
def sanitized_emulator(tmp_path_factory):
    """The same stand-alone program under ASan / UBSan (its own main; nothing of it is loaded into Python)."""
    return _build_emulator(str(tmp_path_factory.mktemp("wavelet_san") / "wavelet_emulate"),
                           ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def gate(got, ref, prefill=None):
    """(elements beyond the gate of the GPU test, largest |got - want| / bound): 1e-6 |ref| + 1e-7 max |ref| + 2^-24 |want|."""
    top = ref.abs().amax(dim=(-3, -2, -1), keepdim=True)
    want = ref if prefill is None else prefill + ref
    bound = 1e-6 * ref.abs() + 1e-7 * top + HALF_ULP * want.abs()
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return int((err > bound).sum()), float(ratio.max())


def _emulate(exe, tmp_path, H, W, rs, Cn, Rr, clamp, vec, name, J, weights, eps, seed=12):
    import numpy as np
    lo, hi = Wv.FILTERS[name]
    scale = 0.37 / (Cn * H * W)
    shape = (1, Cn, H, W)
    x, y = Wv.mixed_pair(shape, seed=seed, R=Rr)
    want_loss, want, want_s, smallest = Wv.value_and_grad(x, y, Rr, bool(clamp), scale, lo, hi, J, weights, eps)
    nan = float("nan")
    xb = torch.full((Cn, H, rs), nan)
    xb[..., :W] = x[0]
    prefill = torch.full((Cn, H, rs), nan)
    prefill[..., :W] = torch.randn(Cn, H, W, generator=torch.Generator().manual_seed(2)) * float(want.abs().max())
    w = list(weights if weights is not None else Wv.default_weights(J)) + [0.0] * 10
    pad = lambda f: list(f) + [0.0] * (8 - len(f))
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("8i", H, W, rs, Cn, clamp, vec, len(lo), J) + struct.pack("f", Rr) + struct.pack("2d", scale, eps))
        f.write(struct.pack("8d", *pad(lo)) + struct.pack("8d", *pad(hi)) + struct.pack("10d", *w[:10]))
        f.write(xb.numpy().tobytes() + y[0].contiguous().numpy().tobytes() + prefill.numpy().tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, capture_output=True)
    b = open(tmp_path / "out.bin", "rb").read()
    nb, ng = 3 * J + 1, 4 * Cn * H * rs
    loss = struct.unpack("f", b[:4])[0]
    sums = torch.tensor(struct.unpack("10d", b[4:84])[:nb], dtype=torch.float64)
    gx = torch.from_numpy(np.frombuffer(b[84:84 + ng], dtype=np.float32).copy()).view(Cn, H, rs)
    swt = torch.from_numpy(np.frombuffer(b[84 + ng:], dtype=np.float32).copy()).view(Cn, nb, H, W)
    assert torch.equal(gx[..., W:].view(torch.int32), prefill[..., W:].view(torch.int32))          # outside [H, W]: bit-unchanged
    got = gx[None, :, :, :W].double()
    nbad, ratio = gate(got, want, prefill[None, :, :, :W].double())
    print(f"emulated kernels {H}x{W} {name} J={J} vec {vec}: largest |got - ref| / bound {ratio:.4f}; value {loss:.9e} against "
          f"{want_loss:.9e}; smallest non-zero |c| {smallest:.3g}")
    assert nbad == 0 and ratio <= 1.0, (nbad, ratio)
    assert float(((sums - want_s).abs() - 1e-12 * want_s.abs()).max()) <= 0.0, (sums, want_s)
    assert abs(loss - want_loss) <= 1.2e-7 * abs(want_loss)
    if clamp:
        keep = (x[0] < 0) | (x[0] > Rr)
        assert int(keep.sum()) > 0 or H * W < 100                  # (four pixels hold no element outside the range)
        assert torch.equal(gx[..., :W][keep].view(torch.int32), prefill[..., :W][keep].view(torch.int32))
    # the transform alone, of x itself: one fp32 rounding of the fp64 coefficient
    d = x[0].double()
    ref = torch.stack(Wv.swt2(d, lo, hi, J), dim=1)
    assert bool(((swt.double() - ref).abs() <= HALF_ULP * ref.abs() + 1e-12 * float(d.abs().max())).all())


@pytest.mark.parametrize("H,W,rs,Cn,Rr,clamp,vec,name,J,weights,eps", [
    (13, 14, 14, 3, 1.0, 1, 1, "db2", 3, None, 0.0),
    (33, 70, 80, 3, 255.0, 1, 1, "haar", 3, None, 0.0),
    (33, 70, 80, 3, 1.0, 1, 1, "db2", 3, [1.0, 0.0, 2.0, 0.5, 1.0, 0.0, 1.0, 1.0, 1.0, 0.25], 1e-3),
    (70, 33, 33, 3, 1.0, 0, 1, "haar", 3, None, 0.0),
    (64, 130, 132, 1, 1.0, 1, 1, "tri", 2, [1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0], 0.0),
    (64, 130, 130, 1, 255.0, 1, 0, "tri", 2, None, 1e-3),
    (2, 2, 2, 1, 1.0, 1, 1, "haar", 1, None, 0.0),
    (29, 40, 40, 1, 1.0, 1, 1, "tap8", 3, [1.0] * 9 + [0.5], 0.0),
    (40, 29, 32, 3, 255.0, 1, 1, "tap8", 2, None, 1e-3)],
    ids=["13x14-db2", "33x70-stride80-haar", "33x70-db2-weights-eps", "70x33-haar", "64x130-tri-level1-only", "64x130-scalar", "2x2",
         "29x40-tap8-min-side", "40x29-tap8"])
def test_kernel_text_emulated_on_the_host_meets_the_gpu_gate(emulator, tmp_path, H, W, rs, Cn, Rr, clamp, vec, name, J, weights, eps):
    """csrc/m2t_wavelet_tile.h -- the text the kernels run -- on host threads (tests/wavelet_emulate.cpp), the kernel's own sum order:
    the shapes of the GPU test, the 16-byte path and the scalar one, x in a NaN-filled buffer with a longer row, a 0xFF-filled scratch;
    both variants of the tile (a reach of at most 12, and -- the 8-tap pair -- of up to 28, at the minimum side where every tap wraps).
    The gradient within the gate of the GPU test, the band sums within 1e-12, the value within fp32 rounding, the bits under the clamp
    kept, nothing written outside [H, W]; the transform alone within one fp32 rounding."""
    _emulate(emulator, tmp_path, H, W, rs, Cn, Rr, clamp, vec, name, J, weights, eps)


@pytest.mark.parametrize("H,W,rs,Cn,Rr,name,J", [(13, 14, 14, 3, 1.0, "db2", 3), (33, 70, 80, 3, 255.0, "haar", 3), (29, 40, 40, 1, 1.0, "tap8", 3)],
                         ids=["13x14-db2", "33x70-stride80-haar", "29x40-tap8"])
def test_kernel_text_is_clean_under_asan_and_ubsan(sanitized_emulator, tmp_path, H, W, rs, Cn, Rr, name, J):
    """The stand-alone emulator built with -fsanitize=address,undefined: every tile, staged halo and LDS index of the text, at the
    minimum side (every level-3 tap wraps) and with a row stride longer than the row; a finding aborts the program."""
    _emulate(sanitized_emulator, tmp_path, H, W, rs, Cn, Rr, 1, 1, name, J, None, 0.0)
