"""CPU test (no GPU): the whole host-side query surface of the C-ABI library, cell for cell.

m2t_plan_create / m2t_set_option / m2t_plan_query and the Swin / BERT create and query calls allocate nothing on a device.
`walk()` sets a fixed lattice of plans and options and records the answer to every query key; the test compares that table
for EQUALITY with tests/golden/plan_surface.npz, which the same walker wrote from the library of the commit BEFORE the
schedule / layout-table refactor of the host layer:

    python tests/test_plan_surface_cpu.py --write /path/to/parent/libm2t.so

(never from the code under test).  The lattice:
  * full product at (B, H0, W0, nb) = (2, 40, 56, 2) over dtype {fp32, bf16} x scale {2, 3, 4} x fused_tail 0..4 x attn_bwd 0..3
    x fused_attn_fwd 0..2 x fused_c16_fwd 0..2 x {fused_prep_fwd, fused_prep_bwd, fused_norm_red, fused_l1, tail_bwd_mfma32}
    in {0, 1}: 5 760 settings on each of 6 plans;
  * one at a time from the default, every other option over its whole range, on each (dtype, scale) at (2, 40, 56),
    (16, 192, 192) (576 windows at the C = 256 level, even window grid) and (32, 96, 160) (480 windows, odd 3 x 5 grid);
  * per setting: every opt:* key, the four stores_* keys and workspace_bytes;
  * the return code of m2t_set_option for one out-of-range value per ranged option and for an unknown key;
  * the layout inventory (param: / numel: / ws: / wsn: / packed: / grad buckets) of each (dtype, scale) plan at the small shape and
    of m2t_swin_create(8, bf16) and m2t_text_create(8, 77, bf16), including the key families a handle answers -1 for.
"""
import ctypes as C
import itertools
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_surface.npz")

OPT_KEYS = ("side_stream", "fork_on_kernel", "fp32_fast", "tail_bwd_mfma32", "fused_l1", "fused_attn_fwd2", "fused_norm_red",
            "fused_prep_fwd", "fused_prep_bwd", "gate_branch", "wgrad_big_tiles", "fused_tail", "attn_bwd", "conv_rows",
            "fused_conv_bwd", "fused_attn_fwd", "fused_c16_fwd", "fused_qkv_dgrad", "debug_skip_side", "no_such_option")
KEYS = tuple("opt:" + k for k in OPT_KEYS) + ("stores_qkv1", "stores_qkv2", "stores_t1", "stores_t2", "workspace_bytes")
PRODUCT = (("fused_tail", range(5)), ("attn_bwd", range(4)), ("fused_attn_fwd", range(3)), ("fused_c16_fwd", range(3)),
           ("fused_prep_fwd", (0, 1)), ("fused_prep_bwd", (0, 1)), ("fused_norm_red", (0, 1)), ("fused_l1", (0, 1)),
           ("tail_bwd_mfma32", (0, 1)))
SINGLE = (("side_stream", (0, 1)), ("fork_on_kernel", (0, 1)), ("fp32_fast", (0, 1)), ("conv_rows", (0, 1)),
          ("fused_conv_bwd", (0, 1)), ("gate_branch", (-1, 0, 1, 2, 3)), ("wgrad_big_tiles", (-1, 0, 256)),
          ("debug_skip_side", (0, 1)), ("fused_attn_fwd2", (-1, 0, 1, 2)))
REJECTED = (("fused_tail", 5), ("attn_bwd", 4), ("fused_attn_fwd", 3), ("fused_c16_fwd", 3), ("conv_rows", 2), ("gate_branch", 4),
            ("fused_attn_fwd2", 3), ("no_such_option", 1))
SMALL, SHAPES = (2, 40, 56), ((2, 40, 56), (16, 192, 192), (32, 96, 160))
NB = 2
PLANS = tuple(itertools.product((0, 1), (2, 3, 4)))      # (dtype: 0 = fp32, 1 = bf16, scale)


def load_library(path):
    from m2trans_amd import _lib
    import torch  # noqa: F401  (its HIP runtime first, as _lib.load does)
    lib = C.CDLL(path)
    for name, (res, args) in _lib.ABI["m2t.h"].items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def _plan(lib, dt, scale, shape):
    h = C.c_void_p()
    assert lib.m2t_plan_create(C.byref(h), shape[0], shape[1], shape[2], scale, NB, dt) == 0
    return h


def _plan_inventory(lib, h, dt, scale):
    """[query answers] over parameter, workspace, pack and bucket names of one plan (the workspace names are those of the poison
    helper behind test_workspace_region_inventory_is_complete, which also checks that they tile the workspace)."""
    from oracle import m2trans_oracle as O
    from tests.gpu_util import WS_PERSISTENT, ws_float_regions
    q = lambda k: int(lib.m2t_plan_query(h, k.encode()))
    out = [q("num_params"), q("num_param_tensors"), q("padded_h"), q("padded_w"), q("workspace_bytes")]
    for n in list(O.param_shapes(64, scale, NB)) + ["no.such.parameter"]:
        out += [q("param:" + n), q("numel:" + n)]
    shim = types.SimpleNamespace(n_blocks=NB, scale=scale, dtype=dt, query=q)
    for n in [r[0] for r in ws_float_regions(shim)] + list(WS_PERSISTENT) + ["no_such_tensor"]:
        out += [q("ws:" + n), q("wsn:" + n)]
    packs = [f"b{b}.{w}" for b in range(NB) for w in
             [f"w{i}{sfx}" for i in range(1, 5) for sfx in ("", "T", "F", "TF")] + ["wf", "wfT", "wfR", "wfTR"]]
    for n in packs + ["t0", "t0T", "t3", "t3T", "no_such_pack"]:
        out.append(q("packed:" + n))
    nbk = q("grad_buckets")
    out.append(nbk)
    for i in range(nbk + 1):
        out += [q(f"grad_bucket_lo:{i}"), q(f"grad_bucket_hi:{i}")]
    return out


def _encoder_inventory(query, param_name, h, ws_names, pack_names, extra):
    q = lambda k: int(query(h, k.encode()))
    out = [q(k) for k in ("workspace_bytes", "num_params", "num_param_tensors", "grad_buckets", "name:0") + extra]
    n = q("num_param_tensors")
    names = [param_name(h, i).decode() for i in range(n)]
    assert param_name(h, n) is None and param_name(h, -1) is None
    for nm in names + ["no.such.parameter"]:
        out += [q("param:" + nm), q("numel:" + nm)]
    for nm in ws_names + ("no_such_tensor",):
        out += [q("ws:" + nm), q("wsn:" + nm)]
    for nm in pack_names:
        out.append(q("packed:" + nm))
    return out, names


def walk(lib):
    """{array name: integer array} of every recorded answer, in a fixed order."""
    set_opt = lambda h, k, v: lib.m2t_set_option(h, k.encode(), v)
    keys = [k.encode() for k in KEYS]
    rows, settings = [], []

    def record(h, tag):
        settings.append(tag)
        rows.append([lib.m2t_plan_query(h, k) for k in keys])

    inventories, rejected = [], []
    for pi, (dt, scale) in enumerate(PLANS):
        h = _plan(lib, dt, scale, SMALL)
        inventories.append(_plan_inventory(lib, h, dt, scale))
        rejected.append([set_opt(h, k, v) for k, v in REJECTED])
        for values in itertools.product(*(r for _, r in PRODUCT)):
            for (k, _), v in zip(PRODUCT, values):
                assert set_opt(h, k, v) == 0
            record(h, (pi, 0) + values)
        lib.m2t_plan_destroy(h)
        for si, shape in enumerate(SHAPES):
            for oi, (k, rng) in enumerate(SINGLE):
                for v in rng:
                    h = _plan(lib, dt, scale, shape)          # a fresh plan: every other option at its default
                    assert set_opt(h, k, v) == 0
                    record(h, (pi, 1 + si, oi, v) + (0,) * (len(PRODUCT) - 2))
                    lib.m2t_plan_destroy(h)
    table = np.asarray(rows, dtype=np.int64)
    out = {"settings": np.asarray(settings, dtype=np.int16), "workspace_bytes": table[:, -1].copy(),
           "answers": table[:, :-1].astype(np.int16), "rejected": np.asarray(rejected, dtype=np.int32)}
    assert np.array_equal(out["answers"], table[:, :-1])
    for (dt, scale), inv in zip(PLANS, inventories):
        out[f"plan_inventory_{dt}_{scale}"] = np.asarray(inv, dtype=np.int64)
    h = C.c_void_p()
    assert lib.m2t_swin_create(C.byref(h), 8, 1) == 0
    inv, names = _encoder_inventory(lib.m2t_swin_query, lib.m2t_swin_param_name, h,
                                    SWIN_WS,
                                    ("pe", "encoder.layers.0.blocks.0.qkv", "encoder.layers.0.blocks.1.fc1F", "encoder.layers.2.downsample.red"),
                                    ("max_images",))
    out["swin_inventory"] = np.asarray(inv, dtype=np.int64)
    out["swin_names"] = np.frombuffer("\n".join(names).encode(), dtype=np.uint8)
    lib.m2t_swin_destroy(h)
    assert lib.m2t_text_create(C.byref(h), 8, 77, 1) == 0
    inv, names = _encoder_inventory(lib.m2t_text_query, lib.m2t_text_param_name, h,
                                    TEXT_WS, ("encoder.layer.0.qkv", "encoder.layer.11.fc2"), ("max_seqs", "max_len", "max_images"))
    out["text_inventory"] = np.asarray(inv, dtype=np.int64)
    out["text_names"] = np.frombuffer("\n".join(names).encode(), dtype=np.uint8)
    lib.m2t_text_destroy(h)
    return out


SWIN_WS = ("packed", "fbias", "crops", "A0", "X", "Hn", "QKV", "AO", "MH", "emb")               # the names walk() asks the swin handle for
TEXT_WS = ("packed", "fbias", "ids", "mask", "X", "Y", "QKV", "AO", "MH", "pooled")      # the names walk() asks the text handle for


def text_workspace_layout(max_seqs, max_len, es):
    """{region: (byte offset, element count)}, total bytes of the m2t_text workspace, restated from the geometry (BERT-base: 12
    layers of q|k|v, o, fc1, fc2 packs and a fused q|k|v bias) and the rule of m2t_layout.h (each region aligned to 256 bytes):
    since the stage gate of the text tower the handle answers ws: / wsn: (the recorded table, older, holds -1 there) and owns one
    more region, XM."""
    rows, hid, ff = max_seqs * max_len, 768, 3072
    sizes = (("packed", 12 * (4 * hid * hid + 2 * ff * hid), es), ("fbias", 12 * 3 * hid, 4), ("ids", rows, 4), ("mask", rows, 4),
             ("X", rows * hid, es), ("XM", rows * hid, es), ("Y", rows * hid, es), ("QKV", rows * 3 * hid, es), ("AO", rows * hid, es),
             ("MH", rows * ff, es), ("pooled", max_seqs * hid, 4))
    out, off = {}, 0
    for name, n, e in sizes:
        off = (off + 255) & ~255
        out[name] = (off, n)
        off += n * e
    return out, (off + 255) & ~255


def test_plan_query_surface_equals_the_recorded_table():
    from m2trans_amd import _lib
    lib = load_library(_lib.LIB_PATH)
    got = walk(lib)
    assert got["settings"].shape[0] > 30000, "truncated walk"
    want = {k: v for k, v in np.load(GOLDEN).items()}
    assert sorted(want) == sorted(got)
    # text handle (8, 77, bf16): cell 0 (workspace_bytes) and the ws: / wsn: cells are checked against the restated layout, every
    # other cell against the recorded table
    lay, total = text_workspace_layout(8, 77, 2)
    first = 8 + 2 * (int(want["text_inventory"][2]) + 1)
    cells = [0] + list(range(first, first + 2 * len(TEXT_WS)))
    assert [int(v) for v in got["text_inventory"][cells]] == [total] + [v for nm in TEXT_WS for v in lay[nm]]
    assert all(int(v) == -1 for v in want["text_inventory"][cells[1:]])
    got["text_inventory"] = got["text_inventory"].copy()
    got["text_inventory"][cells] = want["text_inventory"][cells]
    h = C.c_void_p()
    assert lib.m2t_text_create(C.byref(h), 8, 77, 1) == 0
    assert (lib.m2t_text_query(h, b"ws:XM"), lib.m2t_text_query(h, b"wsn:XM")) == lay["XM"]
    assert lib.m2t_text_query(h, b"ws:no_such_tensor") == -1 and lib.m2t_text_query(h, b"packed:encoder.layer.0.qkv") == -1
    lib.m2t_text_destroy(h)
    # swin handle (8, bf16): since the stage gate of the image tower it answers wsn: (the recorded table, older, holds -1 there).
    # Those ten cells are checked against the geometry and against the recorded ws: offsets (each region ends, rounded up to 256
    # bytes, where the next begins), every other cell against the recorded table
    inv, rec = got["swin_inventory"], want["swin_inventory"]
    first = 6 + 2 * (int(rec[2]) + 1)
    ws_cells, wsn_cells = list(range(first, first + 2 * len(SWIN_WS), 2)), list(range(first + 1, first + 2 * len(SWIN_WS), 2))
    assert all(int(rec[c]) == -1 for c in wsn_cells) and int(inv[first + 2 * len(SWIN_WS) + 1]) == -1        # wsn:no_such_tensor
    tok = 8 * 3136 * 96
    assert [int(inv[c]) for c in wsn_cells[2:]] == [8 * 3, tok // 2, tok, tok, 3 * tok, tok, 4 * tok, 8 * 512]
    ends = [int(rec[c]) for c in ws_cells[1:]] + [int(rec[0])]
    for c_off, c_n, nm, end in zip(ws_cells, wsn_cells, SWIN_WS, ends):
        es = 4 if nm in ("fbias", "crops", "emb") else 2
        assert (int(rec[c_off]) + int(inv[c_n]) * es + 255) // 256 * 256 == end, nm
    got["swin_inventory"] = inv.copy()
    got["swin_inventory"][wsn_cells] = rec[wsn_cells]
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {bad[0].tolist()}: got {got[name][tuple(bad[0])]}, recorded {want[name][tuple(bad[0])]}"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    assert len(sys.argv) == 3 and sys.argv[1] == "--write", "usage: test_plan_surface_cpu.py --write LIBPATH"
    table = walk(load_library(sys.argv[2]))
    assert table["settings"].shape[0] > 30000
    np.savez_compressed(GOLDEN, **table)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes,", table["settings"].shape[0], "settings")
