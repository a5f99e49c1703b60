"""CPU tests (no GPU) of tiled inference (include/m2t_tiles.h, m2trans_amd/infer.py): the eleventh header against its signature table
and the library's symbols, every argument error of its three entries, the host-only tile grid against the plain-Python grid over a
brute-force range with its properties, the torch restatement the GPU tests compare the kernels with (tests/tiles_ref.py) against
itself, and the command line's four new flags."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import tiles_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -2
BRUTE_T = (1, 2, 8, 32, 33)                                  # every legal overlap, every L up to 4 T + 6
GPU_SHAPES = [(20, 70, 32, 8, 4), (56, 56, 32, 8, 2), (33, 75, 32, 8, 3), (50, 50, 32, 16, 4), (64, 70, 32, 0, 2), (40, 56, 32, 16, 1)]


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_every_argument_error_needs_no_device():
    """Every M2T_ERR_ARG of the three entries is decided on the host before any launch, so it is reported without a device too."""
    from m2trans_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(4096)                                     # never dereferenced: the checks come first
    n, t = C.c_int(-7), C.c_int(-7)
    grid_calls = {
        "null n_out": (70, 32, 8, None, C.byref(t), None), "null tile_len_out": (70, 32, 8, C.byref(n), None, None),
        "L 0": (0, 32, 8, C.byref(n), C.byref(t), None), "L 16385": (16385, 32, 8, C.byref(n), C.byref(t), None),
        "T 0": (70, 0, 0, C.byref(n), C.byref(t), None), "T 16385": (70, 16385, 0, C.byref(n), C.byref(t), None),
        "2 v > T": (70, 32, 17, C.byref(n), C.byref(t), None), "2 v > T, odd T": (70, 33, 17, C.byref(n), C.byref(t), None),
        "v < 0": (70, 32, -1, C.byref(n), C.byref(t), None),
    }
    for what, a in grid_calls.items():
        assert lib.m2t_tile_grid(*a) == ARG, what
    assert (n.value, t.value) == (-7, -7)                      # a refused call writes nothing
    assert b"m2t_tile_grid" in lib.m2t_last_error_string()
    assert lib.m2t_tile_grid(70, 32, 16, C.byref(n), C.byref(t), None) == 0 and (n.value, t.value) == (4, 32)
    assert lib.m2t_tile_grid(16384, 16384, 8192, C.byref(n), C.byref(t), None) == 0 and (n.value, t.value) == (1, 16384)
    # (20, 70, 32, 8): 1 x 3 tiles per image
    gather_calls = {
        "null src": (None, 2, 3, 20, 70, 32, 8, 0, 6, one), "null dst": (one, 2, 3, 20, 70, 32, 8, 0, 6, None),
        "B 0": (one, 0, 3, 20, 70, 32, 8, 0, 1, one), "C 0": (one, 2, 0, 20, 70, 32, 8, 0, 1, one), "B C 65536": (one, 256, 256, 20, 70, 32, 8, 0, 1, one),
        "H 0": (one, 2, 3, 0, 70, 32, 8, 0, 1, one), "W 0": (one, 2, 3, 20, 0, 32, 8, 0, 1, one), "H 16385": (one, 2, 3, 16385, 70, 32, 8, 0, 1, one),
        "W 16385": (one, 2, 3, 20, 16385, 32, 8, 0, 1, one), "T 0": (one, 2, 3, 20, 70, 0, 0, 0, 1, one), "T 16385": (one, 2, 3, 20, 70, 16385, 0, 0, 1, one),
        "2 v > T": (one, 2, 3, 20, 70, 32, 17, 0, 1, one), "v < 0": (one, 2, 3, 20, 70, 32, -1, 0, 1, one),
        "first < 0": (one, 2, 3, 20, 70, 32, 8, -1, 2, one), "count 0": (one, 2, 3, 20, 70, 32, 8, 0, 0, one),
        "first + count past the end": (one, 2, 3, 20, 70, 32, 8, 4, 3, one), "first at the end": (one, 2, 3, 20, 70, 32, 8, 6, 1, one),
        "first + count overflowing an int": (one, 2, 3, 20, 70, 32, 8, 2, 2**31 - 1, one),
    }
    for what, a in gather_calls.items():
        assert lib.m2t_tile_gather(*a, None) == ARG, what
    assert b"m2t_tile_gather" in lib.m2t_last_error_string()
    blend_calls = {
        "null tiles": (None, 2, 3, 20, 70, 32, 8, 4, one, one), "null dst": (one, 2, 3, 20, 70, 32, 8, 4, None, one),
        "B 0": (one, 0, 3, 20, 70, 32, 8, 4, one, None), "C 0": (one, 2, 0, 20, 70, 32, 8, 4, one, None), "B C 65536": (one, 65536, 1, 20, 70, 32, 8, 4, one, None),
        "H 0": (one, 2, 3, 0, 70, 32, 8, 4, one, None), "W 16385": (one, 2, 3, 20, 16385, 32, 8, 1, one, None),
        "T 0": (one, 2, 3, 20, 70, 0, 0, 4, one, None), "T 16385": (one, 2, 3, 20, 70, 16385, 0, 4, one, None),
        "2 v > T": (one, 2, 3, 20, 70, 32, 17, 4, one, None), "v < 0": (one, 2, 3, 20, 70, 32, -1, 4, one, None),
        "scale 0": (one, 2, 3, 20, 70, 32, 8, 0, one, None), "scale 9": (one, 2, 3, 20, 70, 32, 8, 9, one, None),
        "s H above 65536":(one, 1, 1, 16384, 70, 32, 8, 5, one, None),
        "s W above 65536": (one, 1, 1, 20, 8193, 32, 8, 8, one, None),
    }
    for what, a in blend_calls.items():
        assert lib.m2t_tile_blend(*a, None) == ARG, what
    assert b"m2t_tile_blend" in lib.m2t_last_error_string()


# ------------------------------------------------------------------------------------------------------------- the grid
def test_tile_grid_equals_the_python_grid_and_has_its_properties_over_the_brute_force_range():
    from m2trans_amd import infer
    seen = set()
    for T in BRUTE_T:
        for v in range(T // 2 + 1):
            for L in range(1, 4 * T + 7):
                t, o = infer.tile_grid(L, T, v)
                assert (t, o) == R.grid(L, T, v), (L, T, v)
                assert o[0] == 0 and o[-1] == L - t and all(a < b for a, b in zip(o, o[1:])), (L, T, v, o)
                if L <= T:
                    assert (t, o) == (L, [0])
                else:
                    assert t == T and len(o) == -(-(L - T) // (T - v)) + 1
                cov = R.cover(L, T, v)
                assert min(cov) >= 1 and max(cov) <= 3, (L, T, v, cov)
                seen.add(max(cov))
    assert seen == {1, 2, 3}
    with pytest.raises(infer.M2TError):
        infer.tile_grid(70, 32, 17)
    with pytest.raises(infer.M2TError):
        infer.tile_grid(0, 32, 8)


def test_the_gpu_shapes_exercise_what_they_are_listed_for():
    want = {(20, 70, 32, 8, 4): ((1, 20, 1), (3, 32, 2)), (56, 56, 32, 8, 2): ((2, 32, 2), (2, 32, 2)), (33, 75, 32, 8, 3): ((2, 32, 2), (3, 32, 2)),
            (50, 50, 32, 16, 4): ((3, 32, 3), (3, 32, 3)), (64, 70, 32, 0, 2): ((2, 32, 1), (3, 32, 2)), (40, 56, 32, 16, 1): ((2, 32, 2), (3, 32, 3))}
    for (H, W, T, v, s), axes in want.items():
        got = tuple((len(R.grid(L, T, v)[1]), R.grid(L, T, v)[0], max(R.cover(L, T, v))) for L in (H, W))
        assert got == axes, ((H, W, T, v, s), got)
    assert R.grid(33, 32, 8) == (32, [0, 1])                    # the last tile shifted by 1: overlap 31
    assert R.grid(56, 32, 8) == (32, [0, 24])                   # exact fit: nothing shifted
    assert R.grid(64, 32, 0) == (32, [0, 32]) and R.grid(70, 32, 0) == (32, [0, 32, 38])


# ------------------------------------------------------------------------------------------------------------- the restatement
def test_the_weights_are_positive_on_a_tiles_whole_support_and_a_ramp_pair_sums_to_one():
    for T in (1, 2, 8, 33):
        for v in range(T // 2 + 1):
            for L in (1, T, T + 1, 2 * T - v, 3 * T + 5):
                for s in (1, 3):
                    t, o, pairs = R.axis_pairs(L, T, v, s)
                    assert len(pairs) == s * L
                    for here in pairs:
                        assert 1 <= len(here) <= 3 and all(0.0 < w <= 1.0 for _, _, w in here)
                        assert [k for k, _, _ in here] == list(range(here[0][0], here[0][0] + len(here)))
                        if len(here) == 1:
                            assert here[0][2] == 1.0 or len(o) > 1
    # a regular pair of tiles (no shifted tile near): the two ramps sum to 1 over the overlap
    t, o, pairs = R.axis_pairs(56, 32, 8, 2)                    # origins 0, 24: overlap SR 48 .. 63
    for p in range(48, 64):
        (k0, _, w0), (k1, _, w1) = pairs[p]
        assert (k0, k1) == (0, 1) and w0 + w1 == 1.0, p
    assert all(len(pairs[p]) == 1 and pairs[p][0][2] == 1.0 for p in list(range(48)) + list(range(64, 112)))
    # v = 0: the regular seam is a hard cut, only the shifted last tile blends
    t, o, pairs = R.axis_pairs(70, 32, 0, 1)
    assert o == [0, 32, 38] and [len(pairs[p]) for p in (31, 32, 37, 38, 63, 64, 69)] == [1, 1, 1, 2, 2, 1, 1]
    assert pairs[31][0][:2] == (0, 31) and pairs[32][0][:2] == (1, 0) and pairs[32][0][2] == 1.0


@pytest.mark.parametrize("H,W,T,v,s", GPU_SHAPES, ids=["x".join(map(str, c)) for c in GPU_SHAPES])
def test_blending_crops_of_one_image_returns_it_bit_for_bit(H, W, T, v, s):
    g = torch.Generator().manual_seed(H * W + s)
    sr = torch.randn(2, 3, s * H, s * W, generator=g)
    tiles = R.crops(sr, H, W, T, v, s)
    out, var, seam, single = R.blend(tiles, 2, H, W, T, v, s)
    assert out.dtype == torch.float32 and torch.equal(out, sr)
    assert bool(single.any()) and bool((var[:, :, single] == 0).all()) and bool((seam[:, :, single] == 0).all())
    assert float(seam.max()) < 1e-6                              # the tiles agree: what is left is fp64 rounding of m
    # the LR tiles are crops too, and the whole range equals its chunks
    x = torch.randn(2, 3, H, W, generator=g)
    assert torch.equal(R.gather(x, T, v), R.crops(x, H, W, T, v, 1))
    n = R.gather(x, T, v).shape[0]
    assert torch.equal(torch.cat([R.gather(x, T, v, 0, n // 2 + 1), R.gather(x, T, v, n // 2 + 1)]), R.gather(x, T, v))
    # tiles that disagree where they overlap: a positive seam there, 0 in the single-cover zones, the output between the tiles
    if not bool(single.all()):
        noisy = tiles + 0.01 * torch.randn(tiles.shape, generator=g)
        out2, var2, seam2, _ = R.blend(noisy, 2, H, W, T, v, s)
        assert bool((seam2[:, :, single] == 0).all()) and bool((seam2[:, :, ~single] > 0).all())
        assert float((out2 - sr).abs().max()) < 0.1
    # the pointwise stub commutes with cropping
    stub = R.pointwise_stub(s)
    assert torch.equal(R.tiled(stub, x, T, v, 4, s)[0][0], stub(x))


# ------------------------------------------------------------------------------------------------------------- CLI, wrappers
def test_cli_parses_the_tile_flags():
    from m2trans_amd import infer
    base = ["--config", "c.yml", "--model_path", "m.pt", "--input", "in", "--output", "out"]
    a = infer.parse_args(base)
    assert a.tile is None and a.tile_overlap == 16 and a.tile_batch is None and a.seam is None
    a = infer.parse_args(base + ["--tile", "96"])
    assert (a.tile, a.tile_overlap, a.tile_batch, a.seam) == (96, 16, 16, None)
    a = infer.parse_args(base + ["--tile", "96", "--self_ensemble"])
    assert a.tile_batch == 2                                     # 16 views per call
    a = infer.parse_args(base + ["--tile", "32", "--tile_overlap", "8", "--tile_batch", "5", "--seam", "sm", "--self_ensemble", "--spread", "sp"])
    assert (a.tile, a.tile_overlap, a.tile_batch, a.seam, a.spread) == (32, 8, 5, "sm", "sp")
    for bad in (base + ["--seam", "sm"],                         # --seam needs --tile
                base + ["--tile", "32", "--spread", "sp"],       # --spread still needs --self_ensemble
                base + ["--tile", "32", "--tile_overlap", "17"], base + ["--tile", "0"], base + ["--tile", "32", "--tile_batch", "0"],
                base + ["--tile", "x"]):
        with pytest.raises(SystemExit):
            infer.parse_args(bad)


def test_host_tensors_and_gradients_are_refused():
    from m2trans_amd import infer
    x = torch.zeros(1, 3, 40, 40)
    stub = R.pointwise_stub(2)
    for t in (x, x.clone().requires_grad_(True)):
        for call in (lambda: infer.tile_gather(t, 32, 8), lambda: infer.tile_blend(t, 1, 40, 40, 32, 8, 1),
                     lambda: infer.tiled(stub, t, 32, 8), lambda: infer.Tiled(stub, 32, 8, 4)(t)):
            with pytest.raises(infer.M2TError):
                call()
    with pytest.raises(infer.M2TError):
        infer.upscale_folder(stub, "nowhere", "nowhere", seam_dir="sm")        # a seam needs a tile size
