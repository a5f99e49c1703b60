"""Parameter groups and frozen tensors, host side (no GPU): the sixth header against its table and the library, the host-side
validation of the segment-table packer, the resolution of a ``param_groups`` spec against the model's names and offsets, and the
checkpoint shape of a grouped step.  The device side is tests/test_gpu_param_groups.py."""
from __future__ import annotations

import ctypes as C
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M2T_ERR_ARG = -2


def _args(scale=2, nb=2):
    return types.SimpleNamespace(n_feats=64, scale=scale, rgb_range=1.0, n_blocks=nb, colors=3)


def _model(scale=2, nb=2):
    from m2trans_amd.M2Trans_network import create_model
    return create_model(_args(scale, nb))


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_group_and_segment_limits_are_the_headers():
    from m2trans_amd import _lib
    src = open(os.path.join(ROOT, "include", "m2t_groups.h")).read()
    assert f"#define M2T_MAX_GROUPS {_lib.MAX_GROUPS}\n" in src and f"#define M2T_MAX_SEGMENTS {_lib.MAX_SEGMENTS}\n" in src
    assert (_lib.MAX_GROUPS, _lib.MAX_SEGMENTS) == (8, 1024)


def _pack(starts, group, n, n_groups, n_seg=None):
    """(status, blob bytes after the call) with the blob pre-filled with 0xAB."""
    from m2trans_amd import _lib
    lib = _lib.load()
    n_seg = len(group) if n_seg is None else n_seg
    size = max(int(lib.m2t_group_table_bytes(min(max(n_seg, 1), 1024))), 64) + 8 * (len(starts) + len(group))
    blob = C.create_string_buffer(b"\xab" * size, size)
    rc = lib.m2t_group_table_pack((C.c_longlong * len(starts))(*starts), (C.c_int * max(len(group), 1))(*group), n_seg, n, n_groups,
                                  C.cast(blob, C.c_void_p))
    return rc, blob.raw


def test_table_packer_validates_on_the_host_before_writing():
    from m2trans_amd import _lib
    lib = _lib.load()
    assert lib.m2t_group_table_bytes(0) == 0 and lib.m2t_group_table_bytes(1025) == 0 and lib.m2t_group_table_bytes(-1) == 0
    assert lib.m2t_group_table_bytes(1) == 8 * (4 + 2) + 8 and lib.m2t_group_table_bytes(9) == 8 * (4 + 10) + 16
    assert lib.m2t_group_table_bytes(1024) == 8 * (4 + 1025) + 1024
    n = 4099
    good_starts, good_group = [0, 5, 6, 7, 1030, 1031, 2048, 4099], [0, 1, 2, 0, 1, 2, 0]      # segments of length 1 included
    bad = {
        "unsorted": ([0, 5, 7, 6, 1030, 1031, 2048, 4099], good_group, n, 3),
        "an empty segment": ([0, 5, 5, 7, 1030, 1031, 2048, 4099], good_group, n, 3),
        "a gap at the front": ([1, 5, 6, 7, 1030, 1031, 2048, 4099], good_group, n, 3),
        "falls short of n": ([0, 5, 6, 7, 1030, 1031, 2048, 4098], good_group, n, 3),
        "runs past n": ([0, 5, 6, 7, 1030, 1031, 2048, 4100], good_group, n, 3),
        "an id >= n_groups": (good_starts, [0, 1, 2, 0, 1, 3, 0], n, 3),
        "a negative id": (good_starts, [0, 1, -1, 0, 1, 2, 0], n, 3),
        "9 groups": (good_starts, good_group, n, 9),
        "0 groups": (good_starts, good_group, n, 0),
        "1025 segments": (list(range(1026)), [0] * 1025, 1025, 1),
        "n < 1": ([0, 0], [0], 0, 1),
    }
    for what, (starts, group, nn, ng) in bad.items():
        rc, raw = _pack(starts, group, nn, ng)
        assert rc == M2T_ERR_ARG, what
        assert raw == b"\xab" * len(raw), f"{what}: the blob was written"
        assert b"m2t_group_table_pack" in lib.m2t_last_error_string()
    assert lib.m2t_group_table_pack(None, None, 1, 1, 1, None) == M2T_ERR_ARG
    rc, raw = _pack(good_starts, good_group, n, 3)
    assert rc == 0
    q = torch.frombuffer(bytearray(raw[:8 * (4 + 8)]), dtype=torch.int64).tolist()
    assert q == [7, 3, n, 0] + good_starts
    assert list(raw[8 * 12:8 * 12 + 8]) == good_group + [0]                # ids, padded with zeros to a multiple of 8
    assert lib.m2t_group_table_bytes(7) == 8 * 12 + 8
    rc, raw = _pack(list(range(1025)), [i % 8 for i in range(1024)], 1024, 8)      # the limits themselves: 1024 segments of length 1
    assert rc == 0


def test_launching_entries_refuse_bad_scalars_on_the_host():
    """No device is touched: every refusal is decided before a launch (the pointers are non-null and never followed)."""
    from m2trans_amd import _lib
    lib = _lib.load()
    one, tab = C.c_void_p(16), C.c_void_p(64)
    lr, wd, fr = (C.c_float * 8)(*[1e-3] * 8), (C.c_float * 8)(), (C.c_ubyte * 8)()

    def adam(**kw):
        a = dict(p=one, g=one, m=one, v=one, n=8, lr=lr, step=1, ema=None, wd=wd, ema_d=0.0, fr=fr, ng=2, tab=tab, nseg=2)
        a.update(kw)
        return lib.m2t_adam_step_groups(a["p"], a["g"], a["m"], a["v"], a["n"], a["lr"], 0.9, 0.999, 1e-8, a["step"], 1.0, a["ema"],
                                        a["wd"], 0, a["ema_d"], None, a["fr"], a["ng"], a["tab"], a["nseg"], None)

    def norm(**kw):
        a = dict(g=one, n=8, step=1, rec=one, ws=one, fr=fr, ng=2, tab=tab, nseg=2, mx=0.0)
        a.update(kw)
        return lib.m2t_grad_norm_groups(a["g"], a["n"], 1.0, a["mx"], 0, a["step"], 0.9, 0.999, a["rec"], a["ws"], a["fr"], a["ng"],
                                        a["tab"], a["nseg"], None)

    neg = (C.c_float * 8)(*[-1.0] * 8)
    for kw in (dict(n=-1), dict(n=0), dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(lr=None), dict(wd=None),
               dict(fr=None), dict(tab=None), dict(step=0), dict(ng=0), dict(ng=9), dict(nseg=0), dict(nseg=1025), dict(nseg=9),
               dict(ema_d=1.0), dict(wd=neg), dict(p=C.c_void_p(20)), dict(ema=C.c_void_p(24))):
        assert adam(**kw) == M2T_ERR_ARG, kw
    for kw in (dict(n=-1), dict(n=0), dict(g=None), dict(rec=None), dict(ws=None), dict(fr=None), dict(tab=None), dict(step=0),
               dict(ng=0), dict(ng=9), dict(nseg=0), dict(nseg=1025), dict(mx=float("nan"))):
        assert norm(**kw) == M2T_ERR_ARG, kw


# ------------------------------------------------------------------------------------------------------ spec resolution
NO_DECAY = ["*.bias", "*.rel_h", "*.rel_w"]


def test_prefixes_and_suffix_patterns_land_on_the_right_tensors_and_adjacent_tensors_merge():
    from m2trans_amd.param_groups import resolve_param_groups
    m = _model(2, 2)
    names, offs = list(m._names), m.param_offsets()
    assert resolve_param_groups(m, None) is None
    # ("head" next to "*.bias" would claim head.bias twice -- refused, see the error cases: the weights are named themselves)
    g = resolve_param_groups(m, [{"params": ["head.weight"], "lr_scale": 0.1}, {"params": NO_DECAY, "weight_decay": 0.0},
                                 {"params": ["tail.0.weight", "tail.3"], "lr_scale": 2}])
    assert g.n_groups == 4 and g.lr_scale == [0.1, 1.0, 2.0, 1.0] and g.weight_decay == [None, 0.0, None, None]
    assert g.frozen == [False] * 4
    assert g.members[0] == ["head.weight"]
    assert g.members[1] == [n for n in names if n.endswith((".bias", ".rel_h", ".rel_w"))]
    assert "body.1.attn3.rel_w" in g.members[1] and "body.0.feed_forward.0.bias" in g.members[1] and "tail.0.bias" in g.members[1]
    assert g.members[2] == ["tail.0.weight", "tail.3.weight"]
    assert g.members[3] == [n for n in names if n.startswith("body.") and n.endswith(".weight")]      # the implicit default group
    assert sorted(sum(g.members, [])) == sorted(names) and g.group_of == [next(k for k in range(4) if n in g.members[k]) for n in names]
    # the table tiles [0, n) in ascending order; adjacent tensors of one group merge into one segment
    assert g.starts[0] == 0 and g.starts[-1] == m.flat_params.numel() == g.n and g.starts == sorted(set(g.starts))
    assert g.n_seg == len(g.seg_group) < len(names) and all(a != b for a, b in zip(g.seg_group, g.seg_group[1:]))
    o_h, k_h = offs["body.0.attn1.rel_h"]
    o_w, k_w = offs["body.0.attn1.rel_w"]
    o_b, k_b = offs["head.bias"]
    assert o_h == o_b + k_b and o_w == o_h + k_h                       # head.bias | rel_h | rel_w: three tensors, one segment
    assert o_b in g.starts and o_h not in g.starts and o_w not in g.starts and o_w + k_w in g.starts
    for n, grp in zip(names, g.group_of):                                  # every tensor lies inside one segment of its own group
        o, k = offs[n]
        seg = max(i for i, s in enumerate(g.starts[:-1]) if s <= o)
        assert g.seg_group[seg] == grp and o + k <= g.starts[seg + 1], n
    assert g.group_lr(1e-3) == [1e-3 * 0.1, 1e-3, 1e-3 * 2.0, 1e-3] and g.group_weight_decay(0.01) == [0.01, 0.0, 0.01, 0.01]
    assert g.stage_flags == [True] * 4 and not g.any_frozen
    # a dotted prefix stops at a component: "body.1" is not a prefix of "body.10..."; a full name matches itself
    g = resolve_param_groups(_model(2, 2), [{"params": ["body.1", "body.0.attn1.rel_h"], "frozen": True}])
    assert g.members[0] == ["body.0.attn1.rel_h"] + [n for n in names if n.startswith("body.1.")]
    assert g.frozen == [True, False] and g.stage_flags == [True, True, False, True]       # body.0 keeps trainable tensors
    # the packed blob is the library's, for this table
    from m2trans_amd import _lib
    raw = g.pack()
    assert len(raw) == _lib.load().m2t_group_table_bytes(g.n_seg)
    assert torch.frombuffer(bytearray(raw[:8 * (5 + g.n_seg)]), dtype=torch.int64).tolist() == [g.n_seg, 2, g.n, 0] + g.starts


def test_stage_flags_follow_the_frozen_set_like_the_models_own():
    from m2trans_amd.param_groups import resolve_param_groups
    for spec, want in (([{"params": ["head", "body"], "frozen": True}], [False, False, False, True]),
                       ([{"params": ["tail"], "frozen": True}], [True, True, True, False]),
                       ([{"params": ["body"], "frozen": True}], [True, False, False, True]),
                       ([{"params": ["head", "body.0"], "frozen": True}], [False, False, True, True]),
                       ([{"params": ["*.bias"], "frozen": True}], [True, True, True, True])):
        m = _model(2, 2)
        g = resolve_param_groups(m, spec)
        frozen = set(g.frozen_names())
        assert g.stage_flags == want == m.stage_flags([n not in frozen for n in m._names]), spec
        for n, p in m._trainable():
            p.requires_grad_(n not in frozen)
        assert m.stage_flags() == want
        r = resolve_param_groups(m, "requires_grad")                         # "requires_grad" follows the flags
        assert set(r.frozen_names()) == frozen and r.stage_flags == want and r.spec == "requires_grad"
        assert r.frozen == [True, False] and r.starts == g.starts and r.seg_group == g.seg_group
    m = _model(2, 1)
    r = resolve_param_groups(m, "requires_grad")                             # nothing frozen: the default group alone
    assert r.n_groups == 1 and r.n_seg == 1 and r.starts == [0, m.flat_params.numel()] and not r.any_frozen


def test_spec_errors_raise_at_resolution():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.param_groups import resolve_param_groups
    m = _model(2, 2)
    with pytest.raises(M2TError, match="matched by entries 0 and 1"):
        resolve_param_groups(m, [{"params": ["head"]}, {"params": ["*.bias"]}])
    with pytest.raises(M2TError, match="matches no trainable tensor"):
        resolve_param_groups(m, [{"params": ["body.2"]}])
    with pytest.raises(M2TError, match="matches no trainable tensor"):
        resolve_param_groups(m, [{"params": ["sub_mean"]}])                  # the MeanShift tensors are not in the flat buffer
    nine = [{"params": [n]} for n in m._names[:8]]
    with pytest.raises(M2TError, match="9 groups"):
        resolve_param_groups(m, nine)                                        # 8 explicit + the implicit default group
    assert resolve_param_groups(m, nine[:7]).n_groups == 8
    for bad in (-0.1, float("nan"), float("inf"), "x"):
        with pytest.raises(M2TError, match="lr_scale"):
            resolve_param_groups(m, [{"params": ["tail"], "lr_scale": bad}])
        with pytest.raises(M2TError, match="weight_decay"):
            resolve_param_groups(m, [{"params": ["tail"], "weight_decay": bad}])
    with pytest.raises(M2TError, match="every tensor is frozen"):
        resolve_param_groups(m, [{"params": ["head", "body", "tail"], "frozen": True}])
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(M2TError, match="every tensor is frozen"):
        resolve_param_groups(m, "requires_grad")
    with pytest.raises(M2TError, match="unknown key"):
        resolve_param_groups(m, [{"params": ["tail"], "lr": 1e-3}])
    with pytest.raises(M2TError, match="non-empty list"):
        resolve_param_groups(m, [{"frozen": True}])
    for bad in ("all", 3, [["tail"]]):
        with pytest.raises(M2TError, match="param_groups must be"):
            resolve_param_groups(m, bad)


# ------------------------------------------------------------------------------------------------------------ checkpoint
class _FakeStep:                         # the flat-buffer part of TrainStep, on the CPU
    def __init__(self, m, spec=None, step_count=7, lr=5e-5, **opts):
        from m2trans_amd.param_groups import resolve_param_groups
        self.exp_avg = torch.randn_like(m.flat_params)
        self.exp_avg_sq = torch.rand_like(m.flat_params)
        self.step_count, self.lr, self.betas, self.eps = step_count, lr, (0.9, 0.999), 1e-8
        self.groups = resolve_param_groups(m, spec)
        for k, v in opts.items():
            setattr(self, k, v)

    def set_lr(self, lr):
        self.lr = lr


def test_checkpoint_with_groups_has_one_torch_group_per_group_and_no_state_for_frozen_tensors():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.checkpoint import export_checkpoint, import_checkpoint
    m = _model(2, 2)
    names = list(m._names)
    # (the "body" prefix would overlap "*.bias": the frozen group names the body's weights)
    spec = [{"params": ["head.weight"], "lr_scale": 0.1}, {"params": NO_DECAY, "weight_decay": 0.0},
            {"params": [n for n in names if n.startswith("body.") and n.endswith(".weight")], "frozen": True}]
    fs = _FakeStep(m, spec, weight_decay=0.01, decoupled_weight_decay=True)
    ck = export_checkpoint(m, fs, epoch=3)
    od = ck["optimizer_state_dict"]
    pgs = od["param_groups"]
    assert len(pgs) == 4 == fs.groups.n_groups
    assert [pg["lr"] for pg in pgs] == [5e-5 * 0.1, 5e-5, 5e-5, 5e-5]
    assert [pg["weight_decay"] for pg in pgs] == [0.01, 0.0, 0.01, 0.01]
    assert all(pg["decoupled_weight_decay"] for pg in pgs)
    n_extra = len(list(m.named_parameters())) - len(names)                  # the frozen MeanShift tensors, at the end of the last group
    assert [len(pg["params"]) for pg in pgs] == [len(x) for x in fs.groups.members[:3]] + [len(fs.groups.members[3]) + n_extra]
    assert [i for pg in pgs for i in pg["params"]] == list(range(len(names) + n_extra))
    order = [n for mem in fs.groups.members for n in mem]
    frozen = set(fs.groups.frozen_names())
    assert frozen and set(od["state"]) == {i for i, n in enumerate(order) if n not in frozen}
    offs = m.param_offsets()
    for i, n in enumerate(order):
        if n not in frozen:
            o, k = offs[n]
            assert torch.equal(od["state"][i]["exp_avg"].reshape(-1), fs.exp_avg[o:o + k]) and float(od["state"][i]["step"]) == 7.0
    mg = ck["m2t_groups"]
    assert mg["spec"] == fs.groups.spec and mg["groups"] == fs.groups.describe()
    assert (mg["lr"], mg["weight_decay"], mg["decoupled_weight_decay"]) == (5e-5, 0.01, True)
    assert ck["scheduler_state_dict"]["_last_lr"] == [pg["lr"] for pg in pgs]
    # a stock torch Adam built with the same four groups accepts the state
    by = dict(m.named_parameters())
    extra = [p for n, p in m.named_parameters() if n not in set(names)]
    tg = [{"params": [by[n] for n in mem] + (extra if gi == 3 else [])} for gi, mem in enumerate(fs.groups.members)]
    torch.optim.Adam(tg, lr=1e-4).load_state_dict(od)
    # import: the same spec loads; frozen tensors come back with zero moments; the step's own lr and decay are restored
    m2 = _model(2, 2)
    fs2 = _FakeStep(m2, spec, lr=1.0, weight_decay=0.5, decoupled_weight_decay=False)
    assert import_checkpoint(ck, m2, fs2) == 4
    assert fs2.step_count == 7 and fs2.lr == 5e-5 and fs2.weight_decay == 0.01 and fs2.decoupled_weight_decay is True
    for n in names:
        o, k = offs[n]
        if n in frozen:
            assert not fs2.exp_avg[o:o + k].any() and not fs2.exp_avg_sq[o:o + k].any(), n
        else:
            assert torch.equal(fs2.exp_avg[o:o + k], fs.exp_avg[o:o + k]) and torch.equal(fs2.exp_avg_sq[o:o + k], fs.exp_avg_sq[o:o + k]), n
    # another spec, or none, is refused with the difference named
    other = [dict(spec[0], lr_scale=0.2), spec[1], spec[2]]
    with pytest.raises(M2TError, match="group 0: lr_scale 0.1 against 0.2"):
        import_checkpoint(ck, _model(2, 2), _FakeStep(m2, other))
    with pytest.raises(M2TError, match="holds other tensors"):
        import_checkpoint(ck, m2, _FakeStep(m2, [spec[0], spec[1], {"params": ["tail.3"], "frozen": True}]))
    with pytest.raises(M2TError, match="4 groups against 2"):
        import_checkpoint(ck, m2, _FakeStep(m2, [spec[0]]))
    with pytest.raises(M2TError, match="built without parameter groups"):
        import_checkpoint(ck, m2, _FakeStep(m2))
    with pytest.raises(M2TError, match="written without parameter groups"):
        import_checkpoint(export_checkpoint(m, _FakeStep(m), epoch=3), m2, _FakeStep(m2, spec))


def test_the_group_free_export_is_unchanged():
    from m2trans_amd.checkpoint import export_checkpoint
    m = _model(4, 1)
    torch.manual_seed(5)
    fs = _FakeStep(m)
    ck = export_checkpoint(m, fs, epoch=3)
    assert list(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "stat_dict"]
    od = ck["optimizer_state_dict"]
    assert len(od["param_groups"]) == 1 and od["param_groups"][0]["lr"] == 5e-5 and od["param_groups"][0]["weight_decay"] == 0
    n_all = len(list(m.named_parameters()))
    assert od["param_groups"][0]["params"] == list(range(n_all)) and len(od["state"]) == len(m._names)
    del fs.groups                                                           # a step object that knows no groups exports the same
    ck2 = export_checkpoint(m, fs, epoch=3)
    assert list(ck2) == list(ck) and ck2["optimizer_state_dict"]["param_groups"] == od["param_groups"]
    assert all(torch.equal(ck2["optimizer_state_dict"]["state"][i]["exp_avg"], od["state"][i]["exp_avg"]) for i in od["state"])
