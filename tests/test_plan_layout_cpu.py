"""CPU test (no GPU): the workspace layout of a plan in every mode, cell for cell.

m2t_plan_create / m2t_set_option / m2t_plan_query allocate nothing on a device.  `walk()` sets a fixed lattice of plans, modes and
options and records every layout answer; the test compares the table for EQUALITY with tests/golden/plan_layout_surface.npz, which
the same walker wrote from the library of the commit BEFORE the three layout lists of the host layer (training, inference, health)
became readers of one region table:

    python tests/test_plan_layout_cpu.py --write /path/to/parent/libm2t.so

(never from the code under test).  tests/test_plan_surface_cpu.py covers default training plans only; this one covers the modes.
The lattice, at (B, H0, W0) = (2, 40, 56) (padded, non-square):
  * plans: dtype {fp32, bf16} x scale {2, 3, 4} x depth {1, 2, 3, 8} (depth 3: the smallest at which an inference X3 aliases X1);
  * modes: training; inference; inference with local_norm 8 and 64; health 1 and 2;
  * options per mode: the six settings of test_lean_plan_cpu.test_layout_invariants, then fused_tail 0..4 and attn_bwd 0..3 one at
    a time; settings with an even index are made after the mode, those with an odd index before it;
  * per setting: workspace_bytes; ws: / wsn: of every name a training plan knows, of the local-norm and health regions and of one
    unknown name; health_rows; per row its name (health_name:<i> + m2t_last_error_string, as an index into the name list), the
    length that query answers and health_phase:<i>; health_row:<name> of every workspace name, "sr" and "grads";
  * transitions, recorded after every step, whose last state must also equal a fresh plan with the same options;
  * the return codes of the refused combinations.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_layout_surface.npz")

SHAPE = (2, 40, 56)
DEPTHS = (1, 2, 3, 8)
PLANS = tuple(itertools.product((0, 1), (2, 3, 4), DEPTHS))      # (dtype: 0 = fp32, 1 = bf16, scale, depth)
MODES = ((), (("inference", 1),), (("inference", 1), ("local_norm", 8)), (("inference", 1), ("local_norm", 64)), (("health", 1),),
         (("health", 2),))
SETTINGS = ((), (("fused_attn_fwd", 0), ("fused_c16_fwd", 0), ("fused_tail", 0)), (("fused_prep_fwd", 0),), (("fused_attn_fwd2", 1),),
            (("fused_attn_fwd", 1), ("fused_c16_fwd", 1)), (("fused_tail", 2),)) + tuple(
                ((k, v),) for k, rng in (("fused_tail", range(5)), ("attn_bwd", range(4))) for v in rng)
# (the steps, the options of the fresh plan the last state must equal)
TRANSITIONS = (((("inference", 1), ("inference", 0)), ()),
               ((("health", 2), ("health", 0)), ()),
               ((("health", 1), ("fused_tail", 0), ("health", 0), ("fused_tail", 3)), (("fused_tail", 3),)),
               ((("inference", 1), ("local_norm", 64), ("local_norm", 0), ("inference", 0)), ()),
               ((("inference", 1), ("fused_attn_fwd", 0), ("inference", 0), ("health", 2)), (("fused_attn_fwd", 0), ("health", 2))))
# (options set first, each accepted; then the refused call)
REFUSED = (((("health", 1),), ("inference", 1)), ((("health", 2),), ("inference", 1)),
           ((("inference", 1),), ("health", 1)), ((("inference", 1),), ("health", 2)), ((("inference", 1),), ("health_on", 0)),
           ((("inference", 1),), ("health_on", 1)), ((), ("local_norm", 8)), ((), ("local_norm", 64)), ((), ("local_norm", 7)),
           ((("inference", 1),), ("local_norm", 7)), ((("inference", 1),), ("local_norm", 16385)), ((("inference", 1),), ("local_norm", -1)),
           ((("inference", 1), ("local_norm", 8)), ("inference", 0)), ((), ("health", 3)), ((), ("health", -1)), ((), ("health_on", 2)))
EXTRA = ("xn", "lnsum", "norm_id", "health", "health_part", "health_descs", "health_work", "no_such_tensor")
MIN_RECORDS = len(PLANS) * (len(MODES) * len(SETTINGS) + sum(len(steps) + 1 for steps, _ in TRANSITIONS))


def ws_names(nb):
    """Every workspace name a training plan of this depth knows (the x4-only names are asked at every scale), then EXTRA."""
    from tests.test_lean_plan_cpu import all_names
    names = all_names(nb, 4)
    assert len(set(names)) == len(names) and not set(names) & set(EXTRA)
    return names + list(EXTRA)


def record(lib, h, nb):
    """[every layout answer of the plan as it stands], [a label per answer]"""
    q = lambda k: int(lib.m2t_plan_query(h, k.encode()))
    names = ws_names(nb)
    vocab = {n: i for i, n in enumerate(names + ["sr", "grads"])}
    keys = ["workspace_bytes"] + [f"{f}:{n}" for n in names for f in ("ws", "wsn")] + ["health_rows"]
    out = [q(k) for k in keys]
    for i in range(out[-1] + 1):             # (one past the last row: the out-of-range answers)
        n = q(f"health_name:{i}")
        name = lib.m2t_last_error_string().decode() if n >= 0 else ""
        out += [vocab.get(name, -2) if n >= 0 else -1, n, q(f"health_phase:{i}")]
        keys += [f"health_name:{i} (index into the name list)", f"health_name:{i} (length)", f"health_phase:{i}"]
    rows = [f"health_row:{n}" for n in names + ["sr", "grads"]]
    return out + [q(k) for k in rows], keys + rows


def _plan(lib, dt, scale, nb, opts=()):
    h = C.c_void_p()
    assert lib.m2t_plan_create(C.byref(h), SHAPE[0], SHAPE[1], SHAPE[2], scale, nb, dt) == 0
    for k, v in opts:
        assert lib.m2t_set_option(h, k.encode(), v) == 0, (k, v)
    return h


def walk(lib):
    """{array name: integer array} of every recorded answer, in a fixed order, and the labels of every record."""
    records, labels, tags, refused = [], [], [], []

    def take(h, nb, tag):
        r, l = record(lib, h, nb)
        records.append(r)
        labels.append((tag, l))
        tags.append(tag)
        return r

    for pi, (dt, scale, nb) in enumerate(PLANS):
        for mi, mode in enumerate(MODES):
            for si, setting in enumerate(SETTINGS):
                h = _plan(lib, dt, scale, nb, mode + setting if si % 2 == 0 else setting + mode)
                take(h, nb, (pi, 0, mi, si))
                lib.m2t_plan_destroy(h)
        for ti, (steps, fresh) in enumerate(TRANSITIONS):
            h = _plan(lib, dt, scale, nb)
            for si, (k, v) in enumerate(steps):
                assert lib.m2t_set_option(h, k.encode(), v) == 0, (k, v)
                last = take(h, nb, (pi, 1, ti, si))
            lib.m2t_plan_destroy(h)
            h = _plan(lib, dt, scale, nb, fresh)
            assert take(h, nb, (pi, 1, ti, len(steps))) == last, f"plan {(dt, scale, nb)}: transition {ti} does not end in the state of a fresh plan"
            lib.m2t_plan_destroy(h)
        codes = []
        for first, (k, v) in REFUSED:
            h = _plan(lib, dt, scale, nb, first)
            before = record(lib, h, nb)[0]
            codes.append(lib.m2t_set_option(h, k.encode(), v))
            assert codes[-1] != 0 and record(lib, h, nb)[0] == before, f"plan {(dt, scale, nb)}: {first} then {(k, v)}"
            lib.m2t_plan_destroy(h)
        refused.append(codes)
    out = {"tags": np.asarray(tags, dtype=np.int16), "lengths": np.asarray([len(r) for r in records], dtype=np.int32),
           "answers": np.asarray([v for r in records for v in r], dtype=np.int64), "refused": np.asarray(refused, dtype=np.int32)}
    return out, labels


def load_library(path):
    from tests.test_plan_surface_cpu import load_library as load
    return load(path)


def test_plan_layout_surface_equals_the_recorded_table():
    from m2trans_amd import _lib
    got, labels = walk(load_library(_lib.LIB_PATH))
    assert got["tags"].shape[0] >= MIN_RECORDS == 2664, "truncated walk"
    want = {k: v for k, v in np.load(GOLDEN).items()}
    assert sorted(want) == sorted(got)
    for name in ("tags", "lengths", "refused", "answers"):
        assert got[name].dtype == want[name].dtype, name
        if got[name].shape == want[name].shape and np.array_equal(got[name], want[name]):
            continue
        if name == "answers":          # (tags and lengths are equal here: the records line up)
            cell = int(np.argmax(got[name] != want[name]))
            ends = np.cumsum(got["lengths"])
            rec = int(np.searchsorted(ends, cell, side="right"))
            pos = cell - (int(ends[rec - 1]) if rec else 0)
            (pi, kind, a, b), keys = labels[rec]
            where = f"mode {MODES[a]} setting {SETTINGS[b]} ({'after' if b % 2 == 0 else 'before'} the mode)" if kind == 0 else \
                f"transition {TRANSITIONS[a][0]} after step {b}"
            raise AssertionError(f"{int(np.sum(got[name] != want[name]))} cells differ, first: plan (dtype, scale, depth) = {PLANS[pi]}, {where}, "
                                 f"{keys[pos]}: got {got[name][cell]}, recorded {want[name][cell]}")
        bad = np.argwhere(got[name] != want[name]) if got[name].shape == want[name].shape else None
        raise AssertionError(f"{name}: shape {got[name].shape} against {want[name].shape}" if bad is None else
                             f"{name}: {len(bad)} cells differ, first at {bad[0].tolist()}: got {got[name][tuple(bad[0])]}, recorded {want[name][tuple(bad[0])]}")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    assert len(sys.argv) == 3 and sys.argv[1] == "--write", "usage: test_plan_layout_cpu.py --write LIBPATH"
    table = walk(load_library(sys.argv[2]))[0]
    assert table["tags"].shape[0] >= MIN_RECORDS
    np.savez_compressed(GOLDEN, **table)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes,", table["tags"].shape[0], "records,", table["answers"].shape[0], "answers")
