"""CPU test (no GPU): the grad-workspace surface of the Swin handle, cell for cell.

m2t_swin_grad_workspace_bytes lays the grad workspace for a crop count and caches that layout; the gws: / gwsn: keys of
m2t_swin_query read it.  `walk()` creates m2t_swin_create(max_images, dtype) for max_images in {2, 8} and both dtypes and, on
each handle, asks for n_grad = 1, 2, max_images and 1 again (the last re-lays a layout that was replaced).  After each it records
the returned byte count and the gws: / gwsn: answer for every region name (restated here from the tower's geometry, not asked of
the library) plus one unknown name; before the first call it records that every key answers -1.  The table is compared for
EQUALITY with tests/golden/tower_grad_surface.npz, which the same walker wrote from the library of the commit BEFORE the passes
of the tower stopped looking names up:

    python tests/test_tower_grad_surface_cpu.py --write /path/to/parent/libm2t.so

(never from the code under test).
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tower_grad_surface.npz")
DEPTHS = (2, 2, 6, 2)
HANDLES = tuple((m, dt) for m in (2, 8) for dt in (0, 1))      # (max_images, dtype: 0 = fp32, 1 = bf16)


def grad_region_names():
    """Every region of the grad workspace in the order it is laid, + one name it does not have."""
    names = []
    for s, depth in enumerate(DEPTHS):
        for j in range(depth):
            names += [f"encoder.layers.{s}.blocks.{j}.{k}" for k in ("qkvT", "oT", "fc1T", "fc2T")]
        if s < 3:
            names.append(f"encoder.layers.{s}.downsample.redT")
    names += ["gR", "gF", "gT", "gC", "gQ", "gA", "e0"]
    for s, depth in enumerate(DEPTHS):
        for j in range(depth):
            names += [f"s{s}b{j}.{k}" for k in ("xin", "xmid", "qkv", "gder")]
        if s < 3:
            names.append(f"m{s}")
    return names + ["xf", "hnf", "MD", "no_such_tensor"]


def walk(lib):
    """{array name: int64 array}: per handle one row per step (before the first call, then n_grad = 1, 2, max_images, 1), each row
    [n_grad, returned bytes, then (gws:, gwsn:) per name]."""
    names = grad_region_names()
    out = {"names": np.frombuffer("\n".join(names).encode(), dtype=np.uint8)}
    for max_images, dt in HANDLES:
        h = C.c_void_p()
        assert lib.m2t_swin_create(C.byref(h), max_images, dt) == 0
        q = lambda k: int(lib.m2t_swin_query(h, k.encode()))
        answers = lambda: [v for nm in names for v in (q("gws:" + nm), q("gwsn:" + nm))]
        rows = [[0, 0] + answers()]
        for ng in (1, 2, max_images, 1):
            nbytes = int(lib.m2t_swin_grad_workspace_bytes(h, ng))
            rows.append([ng, nbytes] + answers())
        lib.m2t_swin_destroy(h)
        out[f"swin_{max_images}_{dt}"] = np.asarray(rows, dtype=np.int64)
    return out


def test_swin_grad_workspace_surface_equals_the_recorded_table():
    from m2trans_amd import _lib
    from tests.test_plan_surface_cpu import load_library
    got = walk(load_library(_lib.LIB_PATH))
    want = {k: v for k, v in np.load(GOLDEN).items()}
    assert sorted(want) == sorted(got)
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {bad[0].tolist()}: got {got[name][tuple(bad[0])]}, recorded {want[name][tuple(bad[0])]}"
    # the recorded table itself: -1 everywhere before the first call and for the unknown name; the first and the last step (both
    # n_grad = 1) agree; every known region answers a 256-byte aligned offset inside the returned byte count
    for max_images, dt in HANDLES:
        t = want[f"swin_{max_images}_{dt}"]
        assert (t[0, 2:] == -1).all() and (t[1:, -2:] == -1).all()
        assert (t[1] == t[4]).all()
        assert (t[1:, 2:-2:2] % 256 == 0).all() and (t[1:, 2:-2:2] < t[1:, 1:2]).all() and (t[1:, 3:-2:2] > 0).all()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from tests.test_plan_surface_cpu import load_library
    assert len(sys.argv) == 3 and sys.argv[1] == "--write", "usage: test_tower_grad_surface_cpu.py --write LIBPATH"
    table = walk(load_library(sys.argv[2]))
    np.savez_compressed(GOLDEN, **table)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
