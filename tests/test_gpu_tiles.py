"""-m gpu: tiled inference (k_tiles.hip; m2t_tile_gather, m2t_tile_blend, infer.tiled / Tiled, the --tile flags of the command line)
against the restatement tests/tiles_ref.py.

The gather is a selection and the blend a fixed sequence of single IEEE fp64 operations: every element of both equal to the
restatement, bit for bit.  The seam is compared as the spread of the self-ensemble is: sqrtf of the restated fp32 value, within one
ulp either side (torch.nextafter), and exactly 0 where one tile covers.  The shapes (H, W, T, v, s) are the smallest at which the code
can go wrong:
    (20,70,32,8,4)   one axis with a single short tile, non-square tiles
    (56,56,32,8,2)   exact fit, no shifted tile
    (33,75,32,8,3)   last tile shifted by 1, overlap 31
    (50,50,32,16,4)  triple cover per axis, 9 tiles on a pixel
    (64,70,32,0,2)   v = 0: hard seams plus a blended shifted tile
    (40,56,32,16,1)  scale 1
each with B = 1 and 2, C = 3.  The restated blend runs on the host."""
import json
import os

import numpy as np
import pytest
import torch

from tests import tiles_ref as R

pytestmark = pytest.mark.gpu

GUARD = 67                                                       # elements of canary either side of a buffer (odd: unaligned bases)
SHAPES = [(20, 70, 32, 8, 4), (56, 56, 32, 8, 2), (33, 75, 32, 8, 3), (50, 50, 32, 16, 4), (64, 70, 32, 0, 2), (40, 56, 32, 16, 1)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _lib_():
    from m2trans_amd import _lib
    return _lib, _lib.load()


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _guarded(n, fill):
    """(whole buffer, the n elements between the canaries) on the device."""
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _canaries_hold(buf, n, fill):
    host = buf.cpu()
    return bool((host[:GUARD] == fill).all()) and bool((host[GUARD + n:] == fill).all())


def _within_one_ulp(got, ref):
    lo = torch.nextafter(ref, torch.full_like(ref, -float("inf")))
    hi = torch.nextafter(ref, torch.full_like(ref, float("inf")))
    return bool(((got >= lo) & (got <= hi)).all())


def _tile_shape(B, H, W, T, v, s):
    (th, oy), (tw, ox) = R.grid(H, T, v), R.grid(W, T, v)
    return B * len(oy) * len(ox), s * th, s * tw


# ------------------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("H,W,T,v,s", SHAPES, ids=IDS)
def test_gather_equals_the_restatement_on_every_element(H, W, T, v, s):
    from m2trans_amd.infer import tile_gather
    _lib, lib = _lib_()
    for B in (1, 2):
        x = _rand(B, 3, H, W, seed=H * W + B)
        want = R.gather(x, T, v)
        dx = x.cuda()
        got = tile_gather(dx, T, v)
        assert got.shape == want.shape and torch.equal(got.cpu(), want), B
        n, th, tw = _tile_shape(B, H, W, T, v, 1)
        per = n // B
        # a chunk: for B = 2 it straddles the image boundary; behind canaries, through the C entry itself
        first, count = (per - 1, 2) if B == 2 else (1, per - 1)
        k = count * 3 * th * tw
        buf, dst = _guarded(k, 7.25)
        _lib.check(lib.m2t_tile_gather(_lib.ptr(dx), B, 3, H, W, T, v, first, count, _lib.ptr(dst), _lib.stream_ptr()), "m2t_tile_gather")
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu().view(count, 3, th, tw), want[first:first + count]) and _canaries_hold(buf, k, 7.25), B
        assert torch.equal(tile_gather(dx, T, v, first, count).cpu(), want[first:first + count])
        assert torch.equal(tile_gather(dx, T, v, n - 1).cpu(), want[n - 1:])
        assert torch.equal(dx.cpu(), x)


# ------------------------------------------------------------------------------------------------------------- blend
@pytest.mark.parametrize("H,W,T,v,s", SHAPES, ids=IDS)
def test_blend_equals_the_fp64_restatement_on_every_bit(H, W, T, v, s):
    from m2trans_amd.infer import tile_blend
    _lib, lib = _lib_()
    for B in (1, 2):
        n, sth, stw = _tile_shape(B, H, W, T, v, s)
        tiles = _rand(n, 3, sth, stw, seed=H + W + B)            # tiles that disagree wherever they overlap
        out_r, var_r, seam_r, single = R.blend(tiles, B, H, W, T, v, s)
        assert bool(single.any()) and not bool(single.all()) and float(var_r.max()) > 0.0
        dt = tiles.cuda()
        out, seam = tile_blend(dt, B, H, W, T, v, s, with_seam=True)
        assert tuple(out.shape) == (B, 3, s * H, s * W) and seam.shape == out.shape
        diff = out.cpu() != out_r
        print(f"blend {(H, W, T, v, s)} B={B}: {int(diff.sum())} of {diff.numel()} elements differ from the restatement, "
              f"max |diff| {float((out.cpu() - out_r).abs().max()):.3e}")
        assert torch.equal(out.cpu(), out_r), B
        assert _within_one_ulp(seam.cpu(), seam_r), B
        assert bool((seam.cpu()[:, :, single] == 0).all()) and bool((seam.cpu()[:, :, ~single] > 0).all())
        # a null seam: the same image, and nothing written where a seam would go; both behind canaries
        m = B * 3 * s * H * s * W
        obuf, o2 = _guarded(m, 7.25)
        sbuf, _ = _guarded(m, -3.5)
        _lib.check(lib.m2t_tile_blend(_lib.ptr(dt), B, 3, H, W, T, v, s, _lib.ptr(o2), None, _lib.stream_ptr()), "m2t_tile_blend")
        torch.cuda.synchronize()
        assert torch.equal(o2.cpu().view(out_r.shape), out_r) and _canaries_hold(obuf, m, 7.25) and bool((sbuf == -3.5).all())
        assert torch.equal(tile_blend(dt, B, H, W, T, v, s).cpu(), out_r)
        # with a seam, behind canaries: a second run, bit-identical to the first
        obuf, o3 = _guarded(m, -1.5)
        sbuf, s3 = _guarded(m, -1.5)
        _lib.check(lib.m2t_tile_blend(_lib.ptr(dt), B, 3, H, W, T, v, s, _lib.ptr(o3), _lib.ptr(s3), _lib.stream_ptr()), "m2t_tile_blend")
        torch.cuda.synchronize()
        assert _canaries_hold(obuf, m, -1.5) and _canaries_hold(sbuf, m, -1.5)
        assert torch.equal(o3.view(out.shape), out) and torch.equal(s3.view(out.shape), seam) and torch.equal(dt.cpu(), tiles)


def test_the_wrappers_refuse_what_the_entries_would():
    from m2trans_amd import infer
    x = torch.zeros(2, 3, 40, 56, device="cuda")
    stub = R.pointwise_stub(2)
    bad = [lambda: infer.tile_gather(x, 32, 17), lambda: infer.tile_gather(x, 32, 8, 7, 2), lambda: infer.tile_gather(x, 32, 8, 8),
           lambda: infer.tile_gather(x, 32, 8, 0, 0), lambda: infer.tile_gather(x.double(), 32, 8), lambda: infer.tile_gather(x[:, :, :, ::2], 32, 8),
           lambda: infer.tile_gather(x.clone().requires_grad_(True), 32, 8),
           lambda: infer.tile_blend(torch.zeros(8, 3, 64, 64, device="cuda"), 2, 40, 56, 32, 8, 3),           # another scale
           lambda: infer.tile_blend(torch.zeros(7, 3, 64, 64, device="cuda"), 2, 40, 56, 32, 8, 2),           # a tile short
           lambda: infer.tile_blend(torch.zeros(8, 3, 64, 64, device="cuda").requires_grad_(True), 2, 40, 56, 32, 8, 2),
           lambda: infer.tiled(stub, x.clone().requires_grad_(True), 32, 8), lambda: infer.tiled(stub, x[:, :2].contiguous(), 32, 8),
           lambda: infer.tiled(stub, x, 32, 8, tile_batch=0), lambda: infer.tiled(stub, x, 32, 17),
           lambda: infer.tiled(lambda t: t.double(), x, 32, 8), lambda: infer.tiled(lambda t: t[:, :, :, :4], x, 32, 8)]
    assert tuple(infer.tile_blend(torch.zeros(8, 3, 64, 64, device="cuda"), 2, 40, 56, 32, 8, 2).shape) == (2, 3, 80, 112)
    for call in bad:
        with pytest.raises(infer.M2TError):
            call()
    ups = iter([R.pointwise_stub(2), R.pointwise_stub(3)])      # a second chunk of another scale than the first
    with pytest.raises(infer.M2TError):
        infer.tiled(lambda t: next(ups)(t), x, 32, 8, tile_batch=4)


# ------------------------------------------------------------------------------------------------------------- pointwise stub
@pytest.mark.parametrize("H,W,T,v,s", SHAPES, ids=IDS)
def test_tiled_with_a_pointwise_stub_is_the_stub_on_the_whole_image(H, W, T, v, s):
    """Nearest upsampling times an affine map commutes with cropping: every tile's output is the crop of the whole output, so the
    blend must return that output bit for bit.  A wrong origin, a wrong u or a wrong tile index cannot pass."""
    from m2trans_amd.infer import Tiled, tiled
    stub = R.pointwise_stub(s)
    for B in (1, 2):
        x = _rand(B, 3, H, W, seed=s + B).cuda()
        want = stub(x)
        sr, seam = tiled(stub, x, T, v, tile_batch=5, with_seam=True)
        assert torch.equal(sr, want) and sr.shape == seam.shape
        single = R.blend(R.crops(want.cpu(), H, W, T, v, s), B, H, W, T, v, s)[3]
        assert bool((seam.cpu()[:, :, single] == 0).all()) and float(seam.max()) < 1e-6
        assert torch.equal(tiled(stub, x, T, v, tile_batch=1), want) and torch.equal(Tiled(stub, T, v, 64)(x), want)
    # one tile on both axes: the stub's own output, no other launch; a seam is then all 0
    calls = []
    small = _rand(1, 3, 20, 32, seed=3).cuda()
    got = tiled(lambda t: calls.append(tuple(t.shape)) or stub(t), small, T, v)
    assert calls == [(1, 3, 20, 32)] and torch.equal(got, stub(small))
    sr, seam = tiled(stub, small, T, v, with_seam=True)
    assert torch.equal(sr, stub(small)) and torch.equal(seam, torch.zeros_like(sr))


# ------------------------------------------------------------------------------------------------------------- the real model
class _Counting:
    def __init__(self, model):
        self.model, self.shapes = model, []

    def __call__(self, x):
        self.shapes.append(tuple(x.shape))
        return self.model(x)


_MODELS = {}


def _model(scale, n_blocks, dtype):
    """M2Trans, random init (seeded); built once per (scale, n_blocks, dtype) and never modified."""
    if (scale, n_blocks, dtype) not in _MODELS:
        from m2trans_amd.M2Trans_network import create_model
        from tests.gpu_util import make_args
        torch.manual_seed(4321 + scale)
        _MODELS[(scale, n_blocks, dtype)] = create_model(make_args(scale, n_blocks, dtype)).to("cuda").eval()
    return _MODELS[(scale, n_blocks, dtype)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tiled_model_is_the_hand_composition_on_the_same_chunks(dtype):
    """lr [2,3,64,80], T = 32, v = 8: 3 x 3 tiles per image, 18 in all, in chunks of 8, 8 and 2."""
    from m2trans_amd.infer import SelfEnsemble, Tiled, tiled
    scale, T, v = 4, 32, 8
    model = _Counting(_model(scale, 2, dtype))
    lr = torch.rand(2, 3, 64, 80, generator=torch.Generator().manual_seed(11)).cuda()
    sr, seam = tiled(model, lr, T, v, tile_batch=8, with_seam=True)
    assert model.shapes == [(8, 3, 32, 32), (8, 3, 32, 32), (2, 3, 32, 32)]
    with torch.no_grad():
        (out_r, var_r, seam_r, single), = R.tiled(model.model, lr, T, v, 8, scale, blend_device="cpu")
        plain = model.model(lr)
    assert tuple(sr.shape) == (2, 3, 256, 320) and bool(torch.isfinite(sr).all())
    assert torch.equal(sr.cpu(), out_r)
    assert _within_one_ulp(seam.cpu(), seam_r) and bool((seam.cpu()[:, :, single] == 0).all()) and float(seam.max()) > 0.0
    assert not torch.equal(sr, plain)                            # the tiles see other statistics than the whole image
    # the chunking does not show in the bits (the forward is bitwise batch-invariant)
    for tb in (1, 18):
        assert torch.equal(tiled(model, lr, T, v, tile_batch=tb), sr), tb
    # a tile that holds the whole image: the model's own output
    model.shapes.clear()
    assert torch.equal(tiled(model, lr, 128, 16), plain) and model.shapes == [(2, 3, 64, 80)]
    # the ensemble per tile: square tiles, ONE call on 8 * tile_batch views per chunk; both outputs blended with the same weights
    model.shapes.clear()
    got = Tiled(SelfEnsemble(model, with_spread=True), T, v, 8)(lr)
    assert model.shapes == [(64, 3, 32, 32), (64, 3, 32, 32), (16, 3, 32, 32)]
    assert isinstance(got, tuple) and len(got) == 2 and got[0].shape == sr.shape and got[1].shape == sr.shape
    with torch.no_grad():
        want = R.tiled(SelfEnsemble(model.model, with_spread=True), lr, T, v, 8, scale, blend_device="cpu")
    assert len(want) == 2 and torch.equal(got[0].cpu(), want[0][0]) and torch.equal(got[1].cpu(), want[1][0])
    assert not torch.equal(got[0], sr) and float(got[1].min()) >= 0.0 and float(got[1].max()) > 0.0


# ------------------------------------------------------------------------------------------------------------- folders, command line
def test_the_command_line_tiles_a_folder_and_writes_the_seam(tmp_path, capsys):
    import yaml
    from PIL import Image
    from m2trans_amd import infer
    scale = 2
    model = _model(scale, 1, "fp32")
    torch.save({"epoch": 1, "model_state_dict": {k: t.detach().cpu().clone() for k, t in model.state_dict().items()}}, tmp_path / "m.pt")
    with open(tmp_path / "c.yml", "w") as f:
        yaml.safe_dump({"model": "M2Trans", "scale": scale, "n_blocks": 1, "n_feats": 64, "colors": 3, "rgb_range": 1.0, "compute_dtype": "fp32"}, f)
    src = tmp_path / "in"
    src.mkdir()
    rng = np.random.default_rng(8)
    sizes = {"b_wide.png": (40, 72), "a_tall.png": (64, 32)}
    for name, (h, w) in sizes.items():
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(src / name)
    base = ["--config", str(tmp_path / "c.yml"), "--model_path", str(tmp_path / "m.pt"), "--input", str(src)]
    out, sm, plain = tmp_path / "out", tmp_path / "seam", tmp_path / "plain"
    assert infer.main(base + ["--output", str(out), "--tile", "32", "--tile_overlap", "8", "--seam", str(sm)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (line["images"], line["tile"], line["tile_overlap"], line["seam"]) == (2, 32, 8, str(sm))
    assert line["self_ensemble"] is False and line["spread"] is None
    factors = json.load(open(sm / "seam.json"))
    assert set(factors["max_seam"]) == set(sizes) and factors["rgb_range"] == 1.0
    for name, (h, w) in sizes.items():
        lr = infer.load_image(src / name, "cuda")
        sr, seam = infer.tiled(model, lr, 32, 8, 16, with_seam=True)
        img = Image.open(out / name)
        assert img.mode == "RGB" and img.size == (w * scale, h * scale)
        assert np.array_equal(np.asarray(img), infer.to_uint8(sr).cpu().numpy())
        grey = seam[0].amax(dim=0, keepdim=True)
        top = float(grey.max())
        assert top > 0.0 and factors["max_seam"][name] == top
        simg = Image.open(sm / name)
        assert simg.mode == "L" and np.array_equal(np.asarray(simg), infer.to_uint8(grey, top).cpu().numpy()[:, :, 0])
    # without --tile: the bytes of the existing path, and None under the new keys
    assert infer.main(base + ["--output", str(plain)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (line["tile"], line["tile_overlap"], line["seam"]) == (None, None, None) and not os.path.exists(plain / "seam.json")
    for name in sizes:
        lr = infer.load_image(src / name, "cuda")
        with torch.no_grad():
            want = infer.to_uint8(model(lr)).cpu().numpy()
        assert np.array_equal(np.asarray(Image.open(plain / name)), want)
        assert not np.array_equal(np.asarray(Image.open(out / name)), want)
    # upscale_folder itself, with the ensemble per tile and both maps
    sp, both = tmp_path / "spread", tmp_path / "both"
    assert infer.upscale_folder(model, src, both, self_ensemble=True, spread_dir=sp, tile=32, overlap=8, seam_dir=tmp_path / "seam2") == sorted(sizes)
    lr = infer.load_image(src / "a_tall.png", "cuda")
    sr, spread, seam = infer.tiled(infer.SelfEnsemble(model, with_spread=True), lr, 32, 8, 2, with_seam=True)
    assert np.array_equal(np.asarray(Image.open(both / "a_tall.png")), infer.to_uint8(sr).cpu().numpy())
    assert json.load(open(sp / "spread.json"))["max_spread"]["a_tall.png"] == float(spread[0].amax(dim=0).max())
    assert json.load(open(tmp_path / "seam2" / "seam.json"))["max_seam"]["a_tall.png"] == float(seam[0].amax(dim=0).max())
    with pytest.raises(infer.M2TError):
        infer.upscale_folder(model, src, plain, seam_dir=sm)     # a seam needs a tile size
