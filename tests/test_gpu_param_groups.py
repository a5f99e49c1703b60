"""Parameter groups and frozen tensors on the device: the grouped Adam pass and the masked gradient norm against the existing,
already-gated m2t_adam_step_ex / m2t_grad_norm, and TrainStep(param_groups=...) against the group-free step.

Every comparison is BIT FOR BIT (int32 / int64 views, so NaN compares too) unless it says otherwise.  The yardstick is never the
new code.  Where a group-free twin is needed it is built with ``track_grad_norm=True``: an option that changes no number but routes
the twin through m2t_adam_step_ex, whose operation sequence the grouped pass restates (the option-free m2t_adam_step forms its bias
correction in fp32 on the host and is a different rounding).

One deviation from the letter of the three-group case: a spec in which ``"head"`` stands next to ``"*.bias"`` claims head.bias
twice, which param_groups refuses by its own rule (a tensor matched by two entries).  The head and tail groups therefore name their
weights; the groups are the same three plus the default one."""
from __future__ import annotations

import ctypes as C
import io

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from tests.gpu_util import build_model, smooth_pair

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-8
ERR_ARG = -2
LR = 1e-3

# ---- the kernel-level table: n = 4099, segments of length 1, boundaries off the 16-byte grid, three groups, group 2 frozen
N = 4099
STARTS = [0, 5, 6, 7, 1030, 1031, 2048, 4099]
SEG_GROUP = [0, 1, 2, 0, 1, 2, 0]
G_LR = [1e-3, 3e-4, 5e-3]
G_WD = [0.01, 0.0, 0.1]                  # (a group without decay next to groups with it: it takes neither decay branch)
G_FROZEN = [0, 0, 1]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _lib():
    from m2trans_amd import _lib
    return _lib


def _table(starts, seg_group, n, n_groups):
    """The device copy of the packed table."""
    L = _lib()
    lib = L.load()
    n_seg = len(seg_group)
    blob = C.create_string_buffer(int(lib.m2t_group_table_bytes(n_seg)))
    rc = lib.m2t_group_table_pack((C.c_longlong * (n_seg + 1))(*starts), (C.c_int * n_seg)(*seg_group), n_seg, n, n_groups,
                                  C.cast(blob, C.c_void_p))
    assert rc == 0
    return torch.frombuffer(bytearray(blob.raw), dtype=torch.uint8).cuda()


def _buffers(n, seed=0, ema=True):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 0.01
    m = torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 1e-4
    e = torch.randn(n, generator=g) if ema else None
    return [None if t is None else t.cuda() for t in (p, gr, m, v, e)]


def _clone(bufs):
    return [None if t is None else t.clone() for t in bufs]


def _workspace():
    return torch.empty(_lib().load().m2t_grad_norm_workspace_bytes() // 8, dtype=torch.float64, device="cuda")


def _grad_norm(g, n, rec, max_norm=0.0, skip=0, step=1):
    L = _lib()
    return L.load().m2t_grad_norm(L.ptr(g), n, 1.0, max_norm, skip, step, B1, B2, L.ptr(rec), L.ptr(_workspace()), L.stream_ptr())


def _grad_norm_groups(g, n, rec, table, n_seg, frozen, max_norm=0.0, skip=0, step=1, n_groups=None):
    L = _lib()
    ng = len(frozen) if n_groups is None else n_groups
    return L.load().m2t_grad_norm_groups(L.ptr(g), n, 1.0, max_norm, skip, step, B1, B2, L.ptr(rec), L.ptr(_workspace()),
                                         (C.c_ubyte * len(frozen))(*frozen), ng, L.ptr(table), n_seg, L.stream_ptr())


def _adam_ex(bufs, n, lr, wd, decoupled, ema_d, rec, step):
    L = _lib()
    p, g, m, v, e = bufs
    return L.load().m2t_adam_step_ex(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, lr, B1, B2, EPS, step, 1.0, L.ptr(e), wd,
                                     int(decoupled), ema_d if e is not None else 0.0, L.ptr(rec), L.stream_ptr())


def _adam_groups(bufs, n, lrs, wds, frozen, table, n_seg, decoupled, ema_d, rec, step, n_groups=None):
    L = _lib()
    p, g, m, v, e = bufs
    ng = len(frozen) if n_groups is None else n_groups
    return L.load().m2t_adam_step_groups(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, (C.c_float * len(lrs))(*lrs), B1, B2, EPS, step,
                                         1.0, L.ptr(e), (C.c_float * len(wds))(*wds), int(decoupled),
                                         ema_d if e is not None else 0.0, L.ptr(rec), (C.c_ubyte * len(frozen))(*frozen), ng,
                                         L.ptr(table), n_seg, L.stream_ptr())


def _zeroed(g, starts, seg_group, frozen):
    z = g.clone()
    for i, grp in enumerate(seg_group):
        if frozen[grp]:
            z[starts[i]:starts[i + 1]] = 0.0
    return z


def _clip_record(g_zeroed, n, step):
    """A record with clip_coef < 1 from the EXISTING norm on the zeroed copy."""
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    assert _grad_norm(g_zeroed, n, rec, max_norm=0.05, skip=1, step=step) == 0
    assert 0.0 < float(rec[2]) < 1.0 and float(rec[3]) == 1.0
    return rec


# =================================================================================================================== kernels
@pytest.mark.parametrize("with_record", [False, True], ids=["norecord", "clip"])
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
@pytest.mark.parametrize("ema", [False, True], ids=["noema", "ema"])
def test_grouped_pass_equals_segmentwise_adam_step_ex(with_record, decoupled, ema):
    step, ema_d = 3, 0.9
    bufs = _buffers(N, seed=1, ema=ema)
    table = _table(STARTS, SEG_GROUP, N, 3)
    rec = _clip_record(_zeroed(bufs[1], STARTS, SEG_GROUP, G_FROZEN), N, step) if with_record else None
    got = _clone(bufs)
    assert _adam_groups(got, N, G_LR, G_WD, G_FROZEN, table, len(SEG_GROUP), decoupled, ema_d, rec, step) == 0
    assert _same(got[1], bufs[1])                                           # the gradient is read only
    for i, grp in enumerate(SEG_GROUP):
        lo, hi = STARTS[i], STARTS[i + 1]
        if G_FROZEN[grp]:
            want = [None if t is None else t[lo:hi] for t in bufs]
        else:
            want = [None if t is None else t[lo:hi].clone() for t in bufs]  # fresh, 16-byte-aligned tensors
            assert all(t is None or t.data_ptr() % 16 == 0 for t in want)
            assert _adam_ex(want, hi - lo, G_LR[grp], G_WD[grp], decoupled, ema_d, rec, step) == 0
            assert not _same(want[0], bufs[0][lo:hi])                       # (the yardstick moved the parameters)
        for k, name in ((0, "p"), (2, "m"), (3, "v"), (4, "ema")):
            if want[k] is not None:
                assert _same(got[k][lo:hi], want[k]), f"segment {i} [{lo},{hi}) group {grp}: {name}"


def test_frozen_ranges_keep_every_bit_and_nan_in_their_gradient_changes_nothing():
    bufs = _buffers(N, seed=2)
    table = _table(STARTS, SEG_GROUP, N, 3)
    rec = _clip_record(_zeroed(bufs[1], STARTS, SEG_GROUP, G_FROZEN), N, 2)
    a = _clone(bufs)
    assert _adam_groups(a, N, G_LR, G_WD, G_FROZEN, table, len(SEG_GROUP), True, 0.9, rec, 2) == 0
    b = _clone(bufs)
    for i, grp in enumerate(SEG_GROUP):
        if G_FROZEN[grp]:
            b[1][STARTS[i]:STARTS[i + 1]] = float("nan")
    assert _adam_groups(b, N, G_LR, G_WD, G_FROZEN, table, len(SEG_GROUP), True, 0.9, rec, 2) == 0
    for k in (0, 2, 3, 4):
        assert _same(a[k], b[k]), k
        for i, grp in enumerate(SEG_GROUP):
            sl = slice(STARTS[i], STARTS[i + 1])
            assert _same(a[k][sl], bufs[k][sl]) == bool(G_FROZEN[grp]), (k, i)
    assert bool(torch.isfinite(b[0]).all())


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 4099])
def test_one_group_of_everything_equals_adam_step_ex(n):
    bufs = _buffers(n, seed=3)
    table = _table([0, n], [0], n, 1)
    got, want = _clone(bufs), _clone(bufs)
    assert _adam_groups(got, n, [2e-3], [0.05], [0], table, 1, True, 0.99, None, 5) == 0
    assert _adam_ex(want, n, 2e-3, 0.05, True, 0.99, None, 5) == 0
    for k in (0, 2, 3, 4):
        assert _same(got[k], want[k]) and not _same(got[k], bufs[k]), k
    got, want = _clone(bufs), _clone(bufs)                                  # coupled decay
    assert _adam_groups(got, n, [2e-3], [0.05], [0], table, 1, False, 0.99, None, 5) == 0
    assert _adam_ex(want, n, 2e-3, 0.05, False, 0.99, None, 5) == 0
    for k in (0, 2, 3, 4):
        assert _same(got[k], want[k]), k


def test_many_short_segments_and_eight_groups_equal_adam_step_ex_group_by_group():
    """600 segments of 1 .. 130 elements over 8 groups, two of them frozen: more segments than one round of the wave-wide lookup
    resolves, several segments inside every workgroup chunk.  Adam is element-wise, so the yardstick is m2t_adam_step_ex on the
    WHOLE buffer with one group's values, read at that group's elements."""
    gen = torch.Generator().manual_seed(7)
    lens = torch.randint(1, 131, (600,), generator=gen).tolist()
    starts = [0]
    for k in lens:
        starts.append(starts[-1] + k)
    n = starts[-1]
    seg_group = [int(x) for x in torch.randint(0, 8, (600,), generator=gen)]
    seg_group = [g if i == 0 or g != seg_group[i - 1] else (g + 1) % 8 for i, g in enumerate(seg_group)]
    lrs = [1e-3 * (i + 1) for i in range(8)]
    wds = [0.0 if i % 3 == 0 else 0.01 * i for i in range(8)]
    frozen = [0, 0, 1, 0, 0, 0, 1, 0]
    owner = torch.empty(n, dtype=torch.long)
    for i, grp in enumerate(seg_group):
        owner[starts[i]:starts[i + 1]] = grp
    owner = owner.cuda()
    bufs = _buffers(n, seed=8)
    table = _table(starts, seg_group, n, 8)
    rec = _clip_record(torch.where(torch.tensor(frozen, device="cuda", dtype=torch.bool)[owner], torch.zeros_like(bufs[1]), bufs[1]), n, 4)
    got = _clone(bufs)
    assert _adam_groups(got, n, lrs, wds, frozen, table, 600, True, 0.9, rec, 4) == 0
    for grp in range(8):
        mine = owner == grp
        assert bool(mine.any())
        want = bufs if frozen[grp] else _clone(bufs)
        if not frozen[grp]:
            assert _adam_ex(want, n, lrs[grp], wds[grp], True, 0.9, rec, 4) == 0
        for k, name in ((0, "p"), (2, "m"), (3, "v"), (4, "ema")):
            assert _same(got[k][mine], want[k][mine]), f"group {grp}: {name}"
        assert _same(got[0][mine], bufs[0][mine]) == bool(frozen[grp])
    masked = torch.zeros(8, dtype=torch.float64, device="cuda")             # the same table through the masked norm
    assert _grad_norm_groups(bufs[1], n, masked, table, 600, frozen, max_norm=0.05, skip=1, step=4) == 0
    assert _same(masked, rec)


def test_a_record_with_applied_zero_writes_nothing():
    bufs = _buffers(N, seed=4)
    bufs[1][10] = float("nan")                                              # a trainable element: the step is skipped
    table = _table(STARTS, SEG_GROUP, N, 3)
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    assert _grad_norm(bufs[1], N, rec, max_norm=0.05, skip=1, step=1) == 0
    assert float(rec[3]) == 0.0 and float(rec[4]) == 1.0
    got = _clone(bufs)
    assert _adam_groups(got, N, G_LR, G_WD, G_FROZEN, table, len(SEG_GROUP), True, 0.9, rec, 1) == 0
    for k in range(5):
        assert _same(got[k], bufs[k]), k


def _norm_table(n):
    if n == 3:
        return [0, 1, 2, 3], [0, 2, 1]
    if n == 1027:
        return [0, 5, 6, 7, 514, 515, 1027], [0, 1, 2, 0, 1, 2]
    return STARTS, SEG_GROUP


@pytest.mark.parametrize("n", [3, 1027, 4099])
@pytest.mark.parametrize("phase", [0, 1], ids=["aligned", "offset1"])
def test_masked_norm_equals_the_norm_of_the_zeroed_copy(n, phase):
    starts, seg_group = _norm_table(n)
    table = _table(starts, seg_group, n, 3)
    gen = torch.Generator().manual_seed(10 + n)
    store = (torch.randn(n + 8, generator=gen) * 0.3).cuda()
    g = store[phase:phase + n]
    assert g.data_ptr() % 16 == 4 * phase
    args = dict(max_norm=0.5, skip=1, step=2)

    def record_of(fn, grad, *a):
        rec = torch.zeros(8, dtype=torch.float64, device="cuda")
        assert fn(grad, n, rec, *a, **args) == 0
        return rec

    zstore = torch.zeros_like(store)                                        # the zeroed copy, at the same 16-byte phase
    zstore[phase:phase + n] = _zeroed(g, starts, seg_group, G_FROZEN)
    want = record_of(_grad_norm, zstore[phase:phase + n])
    got = record_of(_grad_norm_groups, g, table, len(seg_group), G_FROZEN)
    assert _same(got, want), (got.tolist(), want.tolist())
    assert float(got[1]) == 1.0 and float(got[0]) > 0.0
    frozen_idx = torch.zeros(n, dtype=torch.bool)
    for i, grp in enumerate(seg_group):
        if G_FROZEN[grp]:
            frozen_idx[starts[i]:starts[i + 1]] = True
    ref = R.norm64(g.cpu().numpy()[~frozen_idx.numpy()])
    assert abs(float(got[0]) - ref) <= 1e-12 * ref
    pstore = store.clone()                                                  # NaN and Inf in the frozen ranges: no bit changes
    pg = pstore[phase:phase + n]
    pg[frozen_idx.cuda()] = float("nan")
    pg[int(frozen_idx.nonzero()[0])] = float("inf")
    got_p = record_of(_grad_norm_groups, pg, table, len(seg_group), G_FROZEN)
    assert _same(got_p, want) and float(got_p[1]) == 1.0 and float(got_p[3]) == 1.0
    nothing = record_of(_grad_norm_groups, g, table, len(seg_group), [0, 0, 0])     # no frozen group: m2t_grad_norm outright
    assert _same(nothing, record_of(_grad_norm, g))
    assert not _same(nothing, want)


def test_scalar_argument_errors_leave_the_buffers_untouched():
    L = _lib()
    lib = L.load()
    bufs = _buffers(N, seed=6)
    table = _table(STARTS, SEG_GROUP, N, 3)
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    ws = _workspace()
    got = _clone(bufs)
    p, g, m, v, e = got
    lrs, wds, fr = (C.c_float * 3)(*G_LR), (C.c_float * 3)(*G_WD), (C.c_ubyte * 3)(*G_FROZEN)
    st = L.stream_ptr()

    def adam(p=p, g=g, m=m, v=v, n=N, step=1, ng=3, lrs=lrs, tab=table):
        return lib.m2t_adam_step_groups(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, lrs, B1, B2, EPS, step, 1.0, L.ptr(e), wds, 1, 0.9,
                                        None, fr, ng, L.ptr(tab), len(SEG_GROUP), st)

    def norm(g=g, n=N, step=1, ng=3, rec=rec, tab=table):
        return lib.m2t_grad_norm_groups(L.ptr(g), n, 1.0, 0.5, 1, step, B1, B2, L.ptr(rec), L.ptr(ws), fr, ng, L.ptr(tab),
                                        len(SEG_GROUP), st)

    for kw in (dict(n=-1), dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(step=0), dict(ng=0), dict(ng=9), dict(tab=None),
               dict(lrs=None)):
        assert adam(**kw) == ERR_ARG, kw
    for kw in (dict(n=-1), dict(g=None), dict(rec=None), dict(step=0), dict(ng=0), dict(ng=9), dict(tab=None)):
        assert norm(**kw) == ERR_ARG, kw
    assert b"m2t_grad_norm_groups" in lib.m2t_last_error_string()
    torch.cuda.synchronize()
    for k in range(5):
        assert _same(got[k], bufs[k]), k
    assert not rec.any()
    assert adam() == 0 and norm() == 0                                      # (the same calls with good arguments do run)
    assert not _same(got[0], bufs[0]) and float(rec[0]) > 0.0


# ================================================================================================================= TrainStep
CONFIGS = [(2, 2, "bf16"), (2, 2, "fp32"), (4, 1, "bf16")]                  # (the last one: the seed fused into the x4 tail backward)
CONFIG_IDS = ["x2-bf16", "x2-fp32", "x4-fused-tail"]
BATCH, LR_SIDE = 2, 32
BASE = {"track_grad_norm": True}                                            # routes the group-free twin through m2t_adam_step_ex
FROZEN_BODY = [{"params": ["body"], "frozen": True}]
_PARAMS, _PAIRS = {}, {}


def _pair(scale, seed, batch=BATCH):
    key = (scale, seed, batch)
    if key not in _PAIRS:
        x, hr = smooth_pair(batch, LR_SIDE, scale, seed)
        _PAIRS[key] = (x.cuda(), hr.cuda())
    return _PAIRS[key]


def _step_object(cfg, spec=None, **opts):
    from m2trans_amd.train_step import TrainStep
    scale, nb, dtype = cfg
    model, p = build_model(scale, nb, dtype, params=_PARAMS.get((scale, nb)))
    _PARAMS[(scale, nb)] = p
    kw = dict(BASE)
    kw.update(opts)
    return TrainStep(model, lr=LR, world_size=1, param_groups=spec, **kw)


def _state(ts):
    c = lambda t: None if t is None else t.detach().clone()
    return {"p": c(ts.model.flat_params), "m": c(ts.exp_avg), "v": c(ts.exp_avg_sq), "ema": c(ts.ema_params)}


def _ranges(model, pred):
    return [(n, o, k) for n, (o, k) in model.param_offsets().items() if pred(n)]


def _assert_ranges(tag, model, a: dict, b: dict, pred, keys=("p", "m", "v", "ema")):
    rs = _ranges(model, pred)
    assert rs
    for key in keys:
        if a.get(key) is None and b.get(key) is None:
            continue
        bad = [n for n, o, k in rs if not _same(a[key][o:o + k], b[key][o:o + k])]
        assert not bad, f"{tag}: {key} differs in {bad[:6]} ({len(bad)} of {len(rs)} tensors)"


def _assert_changed(tag, model, a: dict, b: dict, pred):
    rs = _ranges(model, pred)
    assert all(not _same(a["p"][o:o + k], b["p"][o:o + k]) for n, o, k in rs), f"{tag}: a trainable tensor did not move"


is_tail = lambda n: n.startswith("tail.")
not_tail = lambda n: not n.startswith("tail.")
is_body = lambda n: n.startswith("body.")
not_body = lambda n: not n.startswith("body.")
everything = lambda n: True


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_tail_only_and_frozen_tail_against_the_full_step(cfg):
    scale = cfg[0]
    x1, hr1 = _pair(scale, 1)
    x2, hr2 = _pair(scale, 2)
    full = _step_object(cfg, ema_decay=0.9)
    tail_only = _step_object(cfg, [{"params": ["head", "body"], "frozen": True}], ema_decay=0.9)
    frozen_tail = _step_object(cfg, [{"params": ["tail"], "frozen": True}], ema_decay=0.9)
    assert tail_only.groups.stage_flags == [False] * (cfg[1] + 1) + [True] and tail_only._need_stage is not None
    assert frozen_tail.groups.stage_flags == [True] * (cfg[1] + 1) + [False]
    s0 = _state(full)
    loss_full = full.step(x1, hr1).clone()
    loss_tail = tail_only.step(x1, hr1).clone()
    loss_ft = frozen_tail.step(x1, hr1).clone()
    s_full, s_tail, s_ft = _state(full), _state(tail_only), _state(frozen_tail)
    m = full.model
    # tail only: head / body keep every bit of p, m, v, ema; the tail is the full step's
    _assert_ranges("tail only, frozen ranges", m, s_tail, s0, not_tail)
    _assert_ranges("tail only, tail", m, s_tail, s_full, is_tail, keys=("p", "m", "v", "ema"))
    _assert_changed("tail only", m, s_tail, s0, is_tail)
    assert _same(loss_tail, loss_full)
    # frozen tail (the deferred seed under a pass whose tail flag is clear): head / body are the full step's, the loss is bit-equal
    _assert_ranges("frozen tail, tail", m, s_ft, s0, is_tail)
    _assert_ranges("frozen tail, head and body", m, s_ft, s_full, not_tail)
    _assert_changed("frozen tail", m, s_ft, s0, not_tail)
    assert _same(loss_ft, loss_full) and bool(torch.isfinite(loss_ft).all()) and float(loss_ft) > 0.0
    # second step: the grouped run's state in a FRESH group-free step object, one step there, the tail ranges again
    fresh = _step_object(cfg, ema_decay=0.9)
    with torch.no_grad():
        fresh.model.flat_params.copy_(tail_only.model.flat_params)
        fresh.exp_avg.copy_(tail_only.exp_avg)
        fresh.exp_avg_sq.copy_(tail_only.exp_avg_sq)
        fresh.ema_params.copy_(tail_only.ema_params)
    fresh.step_count = tail_only.step_count
    assert fresh.step_count == 1
    l_a, l_b = tail_only.step(x2, hr2).clone(), fresh.step(x2, hr2).clone()
    assert _same(l_a, l_b)
    s2 = _state(tail_only)
    _assert_ranges("tail only, second step, tail", m, s2, _state(fresh), is_tail)
    _assert_ranges("tail only, second step, frozen ranges", m, s2, s0, not_tail)
    # the gradient buffer of a frozen tensor reads zeros, not stale memory
    for n, o, k in _ranges(m, not_tail):
        assert not tail_only.grads[o:o + k].any(), n


def _three_groups(model):
    names = list(model._names)
    return [{"params": ["head.weight"], "lr_scale": 0.1},
            {"params": ["*.bias", "*.rel_h", "*.rel_w"], "weight_decay": 0.0},
            {"params": [n for n in names if n.startswith("tail.") and n.endswith(".weight")], "lr_scale": 2}]


THREE_OPTS = dict(weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=0.05, ema_decay=0.9)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_three_groups_and_no_decay_equal_adam_step_ex_tensor_by_tensor(cfg):
    scale = cfg[0]
    probe = _step_object(cfg)
    ts = _step_object(cfg, _three_groups(probe.model), **THREE_OPTS)
    g = ts.groups
    assert g.n_groups == 4 and not g.any_frozen and ts._need_stage is None
    s0 = _state(ts)
    ts.step(*_pair(scale, 1))
    s1 = _state(ts)
    rec = ts.optim_record.clone()
    assert 0.0 < float(rec[2]) < 1.0 and float(rec[3]) == 1.0               # clip_coef < 1, applied
    lrs, wds = g.group_lr(ts.lr), g.group_weight_decay(ts.weight_decay)
    assert lrs == [LR * 0.1, LR, LR * 2.0, LR] and wds == [0.01, 0.0, 0.01, 0.01]
    offs = ts.model.param_offsets()
    for name, grp in zip(ts.model._names, g.group_of):
        o, k = offs[name]
        want = [s0["p"][o:o + k].clone(), ts.grads[o:o + k].clone(), s0["m"][o:o + k].clone(), s0["v"][o:o + k].clone(),
                s0["ema"][o:o + k].clone()]
        assert _adam_ex(want, k, lrs[grp], wds[grp], True, 0.9, rec, 1) == 0
        for key, w in zip(("p", "m", "v", "ema"), (want[0], want[2], want[3], want[4])):
            assert _same(s1[key][o:o + k], w), f"{name} (group {grp}): {key}"


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_grad_norm_with_a_frozen_body_is_the_norm_over_the_trainable_ranges(cfg):
    ts = _step_object(cfg, FROZEN_BODY, max_grad_norm=0.05)
    ts.step(*_pair(cfg[0], 1))
    m = ts.model
    g = ts.grads.detach().cpu().numpy()
    keep = np.zeros(g.size, dtype=bool)
    for n, o, k in _ranges(m, not_body):
        keep[o:o + k] = True
    ref = R.norm64(g[keep])
    assert ref > 0.0 and abs(float(ts.grad_norm) - ref) <= 1e-12 * ref
    z = ts.grads.detach().clone()
    z[torch.from_numpy(~keep).cuda()] = 0.0
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    assert _grad_norm(z, z.numel(), rec, max_norm=0.05, skip=0, step=1) == 0
    assert _same(rec, ts.optim_record), (rec.tolist(), ts.optim_record.tolist())


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_nan_in_the_frozen_ranges_of_both_gradient_buffers_changes_nothing(cfg):
    scale = cfg[0]
    opts = dict(accum_steps=2, skip_nonfinite=True, max_grad_norm=0.05, ema_decay=0.9)
    a, b = _step_object(cfg, FROZEN_BODY, **opts), _step_object(cfg, FROZEN_BODY, **opts)
    assert a.micro_grads is not None and not a.micro_grads.any()           # zero-filled when something is frozen
    x, hr = _pair(scale, 3, batch=2 * BATCH)
    s0 = _state(a)
    for step in range(2):
        for n, o, k in _ranges(a.model, is_body):
            a.grads[o:o + k] = float("nan")
            a.micro_grads[o:o + k] = float("nan")
        la, lb = a.step(x, hr).clone(), b.step(x, hr).clone()
        assert _same(la, lb) and bool(torch.isfinite(la).all())
        _assert_ranges(f"poison step {step + 1}", a.model, _state(a), _state(b), everything)
        assert _same(a.optim_record, b.optim_record)
        assert float(a.skipped_steps) == float(b.skipped_steps) == 0.0 and float(a.optim_record[1]) == 1.0
    _assert_ranges("poison: frozen body", a.model, _state(a), s0, is_body)
    _assert_changed("poison", a.model, _state(a), s0, not_body)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_communication_path_with_one_rank_and_groups_equals_the_plain_path(cfg):
    scale = cfg[0]
    opts = dict(max_grad_norm=0.05, weight_decay=0.01, decoupled_weight_decay=True, ema_decay=0.9, skip_nonfinite=True)
    a = _step_object(cfg, FROZEN_BODY, force_comm_path=True, **opts)
    b = _step_object(cfg, FROZEN_BODY, **opts)
    assert a.overlap_comm and b.bucket is None
    for step in range(1, 3):
        x, hr = _pair(scale, step)
        la, lb = a.step(x, hr).clone(), b.step(x, hr).clone()
        assert _same(la, lb)
        _assert_ranges(f"communication path step {step}", a.model, _state(a), _state(b), everything)
        assert _same(a.optim_record, b.optim_record)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_requires_grad_spec_equals_the_explicit_frozen_body(cfg):
    from m2trans_amd.train_step import TrainStep
    scale, nb, dtype = cfg
    b = _step_object(cfg, FROZEN_BODY, max_grad_norm=0.05)
    model, _ = build_model(scale, nb, dtype, params=_PARAMS[(scale, nb)])
    model.body.requires_grad_(False)
    a = TrainStep(model, lr=LR, world_size=1, param_groups="requires_grad", max_grad_norm=0.05, **BASE)
    assert set(a.groups.frozen_names()) == set(b.groups.frozen_names()) == {n for n in model._names if is_body(n)}
    assert a.groups.stage_flags == b.groups.stage_flags == [True] + [False] * nb + [True]
    s0 = _state(a)
    for step in range(1, 3):
        x, hr = _pair(scale, step)
        assert _same(a.step(x, hr).clone(), b.step(x, hr).clone())
        _assert_ranges(f"requires_grad step {step}", model, _state(a), _state(b), everything)
        assert _same(a.optim_record, b.optim_record)
    _assert_ranges("requires_grad: frozen body", model, _state(a), s0, is_body)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_a_materialised_seed_route_with_a_frozen_body(cfg):
    """lambda_ssim > 0 takes the immediate pixel loss and adds the SSIM term into the seed: that route through m2t_backward_ex."""
    scale = cfg[0]
    full = _step_object(cfg, lambda_ssim=0.1)
    part = _step_object(cfg, FROZEN_BODY, lambda_ssim=0.1)
    s0 = _state(full)
    x, hr = _pair(scale, 1)
    lf, lp = full.step(x, hr).clone(), part.step(x, hr).clone()
    assert _same(lf, lp) and float(full.ssim_loss) > 0.0
    _assert_ranges("ssim route, trainable", full.model, _state(part), _state(full), not_body, keys=("p", "m", "v"))
    _assert_ranges("ssim route, frozen body", full.model, _state(part), s0, is_body, keys=("p", "m", "v"))
    _assert_changed("ssim route", full.model, _state(part), s0, not_body)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_checkpoint_resume_with_groups_is_bit_identical_and_another_spec_is_refused(cfg):
    from m2trans_amd._lib import M2TError
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    scale = cfg[0]
    probe = _step_object(cfg)
    spec = _three_groups(probe.model) + [{"params": ["body.0.attn1.qkv_conv"], "frozen": True}]
    a, b = _step_object(cfg, spec, **THREE_OPTS), _step_object(cfg, spec, **THREE_OPTS)
    for step in range(1, 3):
        x, hr = _pair(scale, step)
        a.step(x, hr), b.step(x, hr)
    buf = io.BytesIO()
    torch.save(export_checkpoint(b.model, b, epoch=1), buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    pgs = ck["optimizer_state_dict"]["param_groups"]
    assert len(pgs) == 5 and [pg["lr"] for pg in pgs] == b.groups.group_lr(LR)
    assert [pg["weight_decay"] for pg in pgs] == [0.01, 0.0, 0.01, 0.01, 0.01] and ck["m2t_groups"]["groups"] == b.groups.describe()
    assert len(ck["optimizer_state_dict"]["state"]) == len(b.model._names) - 1          # none for the frozen tensor
    c = _step_object(cfg, spec, **THREE_OPTS)
    with torch.no_grad():
        c.model.flat_params.mul_(0.5)                                        # (not the weights of the checkpoint)
        c.exp_avg.fill_(1.0)
    c.set_lr(5e-4)
    import_checkpoint(ck, c.model, c)
    assert c.step_count == 2 and c.lr == LR
    x, hr = _pair(scale, 3)
    la, lc = a.step(x, hr).clone(), c.step(x, hr).clone()
    assert _same(la, lc)
    _assert_ranges("resume: third step", a.model, _state(a), _state(c), everything)
    assert _same(a.optim_record, c.optim_record)
    other = _step_object(cfg, spec[:3], **THREE_OPTS)
    with pytest.raises(M2TError, match="parameter groups are not this TrainStep's"):
        import_checkpoint(ck, other.model, other)
    with pytest.raises(M2TError, match="built without parameter groups"):
        import_checkpoint(ck, probe.model, probe)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_one_explicit_group_of_everything_is_the_group_free_step(cfg):
    scale = cfg[0]
    opts = dict(max_grad_norm=0.05, weight_decay=0.01, ema_decay=0.9, skip_nonfinite=True)
    a = _step_object(cfg, [{"params": ["head", "body", "tail"]}], **opts)
    b = _step_object(cfg, **opts)
    assert a.groups.n_groups == 1 and a.groups.n_seg == 1 and a._need_stage is None and b.groups is None
    for step in range(1, 4):
        x, hr = _pair(scale, step)
        assert _same(a.step(x, hr).clone(), b.step(x, hr).clone())
        _assert_ranges(f"one group, step {step}", a.model, _state(a), _state(b), everything)
        assert _same(a.optim_record, b.optim_record)
