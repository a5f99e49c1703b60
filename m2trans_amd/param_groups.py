"""Parameter groups and frozen tensors for TrainStep's fused optimizer (include/m2t_groups.h).

``TrainStep(..., param_groups=spec)`` takes what ``torch.optim.Adam([{"params": ..., "lr": ..., "weight_decay": ...}, ...])`` over a
partly frozen model takes, by NAME:

    spec = "requires_grad"                                   # freeze the trainable tensors whose requires_grad is False
    spec = [{"params": ["head", "body"], "frozen": True}]    # train the tail alone
    spec = [{"params": ["head"], "lr_scale": 0.1},
            {"params": ["*.bias", "*.rel_h", "*.rel_w"], "weight_decay": 0.0},
            {"params": ["tail"], "lr_scale": 2.0}]

``params`` holds state_dict names or dotted prefixes (``"tail"``, ``"body.3"``, ``"body.0.attn1.rel_h"``) and the suffix forms
``"*.bias"`` / ``"*.rel_h"`` / ``"*.rel_w"`` (any ``"*.<last component>"``).  Tensors matched by no entry form an implicit default
group at the end: scale 1, the step's ``weight_decay``, trainable.  A group's learning rate is ``step.lr * lr_scale``; a group
without ``weight_decay`` follows the step's.

This module is pure host code: it resolves a spec against the model's names and offsets (no device needed) into the segment table
of the C ABI -- adjacent tensors of one group merged into one segment -- and the stage flags of m2t_backward_ex.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional

from . import _lib

_KEYS = ("params", "lr_scale", "weight_decay", "frozen")


def _matches(pattern: str, name: str) -> bool:
    if pattern.startswith("*."):
        return name.endswith(pattern[1:])
    return name == pattern or name.startswith(pattern + ".")


def _number(value, what: str) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise _lib.M2TError(f"param_groups: {what} must be a finite number >= 0, got {value!r}") from None
    if not (math.isfinite(v) and v >= 0.0):
        raise _lib.M2TError(f"param_groups: {what} must be a finite number >= 0, got {value!r}")
    return v


class ParamGroups:
    """A resolved spec.  Per group g: ``members[g]`` (tensor names, state_dict order), ``lr_scale[g]``, ``weight_decay[g]`` (None =
    the step's), ``frozen[g]``.  Per trainable tensor (state_dict order): ``group_of``.  The table: ``starts`` (n_seg + 1 bounds) and
    ``seg_group`` (n_seg ids).  ``stage_flags``: m2t_backward_ex's, from the frozen set.  ``spec``: what the caller gave,
    normalised to plain lists / dicts / floats (it goes into checkpoints)."""

    def __init__(self, spec, members, lr_scale, weight_decay, frozen, group_of, starts, seg_group, stage_flags, n):
        self.spec, self.members, self.lr_scale, self.weight_decay, self.frozen = spec, members, lr_scale, weight_decay, frozen
        self.group_of, self.starts, self.seg_group, self.stage_flags, self.n = group_of, starts, seg_group, stage_flags, n

    @property
    def n_groups(self) -> int:
        return len(self.members)

    @property
    def n_seg(self) -> int:
        return len(self.seg_group)

    @property
    def any_frozen(self) -> bool:
        return any(self.frozen)

    def frozen_names(self) -> List[str]:
        return [n for g, names in enumerate(self.members) if self.frozen[g] for n in names]

    def group_lr(self, lr: float) -> List[float]:
        """Each group's learning rate for the step's ``lr``, in Python floats (rounded to fp32 where it crosses the ABI)."""
        return [float(lr) * s for s in self.lr_scale]

    def group_weight_decay(self, weight_decay: float) -> List[float]:
        return [float(weight_decay) if w is None else w for w in self.weight_decay]

    def describe(self) -> list:
        """The resolved groups as plain data: what checkpoints compare (``weight_decay`` None = the step's)."""
        return [{"params": list(self.members[g]), "lr_scale": self.lr_scale[g], "weight_decay": self.weight_decay[g],
                 "frozen": self.frozen[g]} for g in range(self.n_groups)]

    def pack(self) -> bytes:
        """The blob of m2t_group_table_pack (validated by the library on the host); the caller copies it to the device once."""
        lib = _lib.load()
        nbytes = int(lib.m2t_group_table_bytes(self.n_seg))
        if nbytes == 0:
            raise _lib.M2TError(f"param_groups: {self.n_seg} segments (the library takes 1 .. {_lib.MAX_SEGMENTS})")
        blob = C.create_string_buffer(nbytes)
        starts = (C.c_longlong * (self.n_seg + 1))(*self.starts)
        group = (C.c_int * self.n_seg)(*self.seg_group)
        _lib.check(lib.m2t_group_table_pack(starts, group, self.n_seg, self.n, self.n_groups, C.cast(blob, C.c_void_p)),
                   "m2t_group_table_pack")
        return blob.raw


def describe_difference(a: list, b: list) -> Optional[str]:
    """None if two ``describe()`` lists are the same groups, else one sentence naming the first difference."""
    if len(a) != len(b):
        return f"{len(a)} groups against {len(b)}"
    for g, (x, y) in enumerate(zip(a, b)):
        if list(x["params"]) != list(y["params"]):
            only = sorted(set(x["params"]) ^ set(y["params"]))
            return f"group {g} holds other tensors (e.g. {only[:3]})"
        for k in ("lr_scale", "weight_decay", "frozen"):
            if x[k] != y[k]:
                return f"group {g}: {k} {x[k]!r} against {y[k]!r}"
    return None


def resolve_param_groups(model, spec) -> Optional[ParamGroups]:
    """Resolve TrainStep's ``param_groups`` against ``model`` (names, offsets and -- for "requires_grad" -- the flags of its
    trainable tensors).  None for ``spec is None``.  M2TError for: a spec of another form, an unknown key, a tensor matched by two
    entries, a pattern that matches nothing, more than 8 groups, a negative / non-finite lr_scale or weight_decay, everything
    frozen."""
    if spec is None:
        return None
    names = list(model._names)
    if isinstance(spec, str):
        if spec != "requires_grad":
            raise _lib.M2TError(f"param_groups must be None, 'requires_grad' or a list of dicts, got {spec!r}")
        off = [n for n, (_, p) in zip(names, model._trainable()) if not p.requires_grad]
        given, entries = "requires_grad", ([{"params": off, "frozen": True}] if off else [])
    else:
        if not isinstance(spec, (list, tuple)) or not all(isinstance(e, dict) for e in spec):
            raise _lib.M2TError(f"param_groups must be None, 'requires_grad' or a list of dicts, got {spec!r}")
        entries = list(spec)
        given = None
    members, lr_scale, weight_decay, frozen, norm = [], [], [], [], []
    owner = {}
    for gi, e in enumerate(entries):
        unknown = sorted(set(e) - set(_KEYS))
        if unknown:
            raise _lib.M2TError(f"param_groups[{gi}]: unknown key(s) {unknown} (known: {list(_KEYS)})")
        pats = e.get("params")
        if isinstance(pats, str):
            pats = [pats]
        if not pats or not all(isinstance(p, str) for p in pats):
            raise _lib.M2TError(f"param_groups[{gi}]: 'params' must be a non-empty list of names, prefixes or '*.suffix' patterns")
        mine = set()
        for p in pats:
            hit = [n for n in names if _matches(p, n)]
            if not hit:
                raise _lib.M2TError(f"param_groups[{gi}]: {p!r} matches no trainable tensor of the model")
            mine.update(hit)
        for n in mine:
            if n in owner:
                raise _lib.M2TError(f"param_groups: tensor {n!r} is matched by entries {owner[n]} and {gi}")
            owner[n] = gi
        members.append([n for n in names if n in mine])
        lr_scale.append(_number(e.get("lr_scale", 1.0), f"[{gi}] lr_scale"))
        wd = e.get("weight_decay")
        weight_decay.append(None if wd is None else _number(wd, f"[{gi}] weight_decay"))
        frozen.append(bool(e.get("frozen", False)))
        norm.append({"params": list(pats), "lr_scale": lr_scale[-1], "weight_decay": weight_decay[-1], "frozen": frozen[-1]})
    rest = [n for n in names if n not in owner]
    if rest:                                     # the implicit default group, last
        for n in rest:
            owner[n] = len(members)
        members.append(rest)
        lr_scale.append(1.0)
        weight_decay.append(None)
        frozen.append(False)
    if len(members) > _lib.MAX_GROUPS:
        raise _lib.M2TError(f"param_groups: {len(members)} groups (the implicit default group included); at most {_lib.MAX_GROUPS}")
    if all(frozen):
        raise _lib.M2TError("param_groups: every tensor is frozen -- there is nothing to train")
    group_of = [owner[n] for n in names]
    starts, seg_group = [], []
    for (o, k, _), g in zip(model._slots, group_of):
        if k == 0:
            continue
        if not seg_group or seg_group[-1] != g:
            starts.append(o)
            seg_group.append(g)
    n = sum(k for _, k, _ in model._slots)
    starts.append(n)
    if len(seg_group) > _lib.MAX_SEGMENTS:
        raise _lib.M2TError(f"param_groups: {len(seg_group)} segments; at most {_lib.MAX_SEGMENTS}")
    flags = model.stage_flags([not frozen[g] for g in group_of])
    return ParamGroups(given if given is not None else norm, members, lr_scale, weight_decay, frozen, group_of, starts, seg_group,
                       flags, n)
