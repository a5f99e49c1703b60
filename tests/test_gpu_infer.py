"""-m gpu: the inference end (k_infer.hip; m2t_dihedral_pack, m2t_dihedral_merge, m2t_tensor_to_image_u8, m2trans_amd/infer.py,
metrics.evaluate(self_ensemble=True)) against the torch restatement tests/infer_ref.py.

Pack, mean and the 8-bit export are pure selections and single IEEE operations: every element equal to the restatement.  The
variance is compared through the spread: sqrtf of the restated variance, within one ulp either side (torch.nextafter).  The shapes
are the smallest at which the 32 x 32 tile code can go wrong: sides below, at and just over the tile, non-square planes, a single
row, several planes, several tiles."""
import json
import os

import numpy as np
import pytest
import torch

from tests import infer_ref as R

pytestmark = pytest.mark.gpu

ARG = -2
GUARD = 67                                                       # elements of canary either side of a buffer (odd: unaligned bases)
SHAPES = [(3, 17, 40), (6, 33, 31), (3, 32, 32), (1, 1, 70), (3, 64, 64)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _lib_():
    from m2trans_amd import _lib
    return _lib, _lib.load()


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _guarded(n, dtype, fill):
    """(whole buffer, the n elements between the canaries) on the device."""
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _canaries_hold(buf, n, fill):
    host = buf.cpu()
    return bool((host[:GUARD] == fill).all()) and bool((host[GUARD + n:] == fill).all())


def _within_one_ulp(got, ref):
    lo = torch.nextafter(ref, torch.full_like(ref, -float("inf")))
    hi = torch.nextafter(ref, torch.full_like(ref, float("inf")))
    return bool(((got >= lo) & (got <= hi)).all())


# ------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("planes,H,W", SHAPES, ids=IDS)
def test_pack_equals_the_restatement_on_every_element(planes, H, W):
    _lib, lib = _lib_()
    x = _rand(1, planes, H, W, seed=H * W)
    wa, wb = R.pack(x)
    n = 4 * planes * H * W
    src = x.cuda()
    if (planes, H, W) == SHAPES[-1]:                             # dst_b directly behind dst_a: one [8,planes,H,H] batch
        buf = torch.full((2 * n,), 7.25, dtype=torch.float32, device="cuda")
        a, b = buf[:n], buf[n:]
    else:
        a = torch.full((n,), 7.25, dtype=torch.float32, device="cuda")
        b = torch.full((n,), 7.25, dtype=torch.float32, device="cuda")
    _lib.check(lib.m2t_dihedral_pack(_lib.ptr(src), planes, H, W, _lib.ptr(a), _lib.ptr(b), _lib.stream_ptr()), "m2t_dihedral_pack")
    assert torch.equal(a.cpu().view(wa.shape), wa) and torch.equal(b.cpu().view(wb.shape), wb)
    if (planes, H, W) == SHAPES[-1]:
        assert torch.equal(buf.cpu().view(8, planes, H, H), torch.cat([wa, wb]))
    # the wrapper: a batch [N,C,H,W] is N * C planes, view k of image n at batch index (k mod 4) N + n
    from m2trans_amd.infer import dihedral_pack
    x2 = _rand(2, 3, H, W, seed=H + W)
    ga, gb = dihedral_pack(x2.cuda())
    ra, rb = R.pack(x2)
    assert ga.shape == ra.shape and gb.shape == rb.shape and torch.equal(ga.cpu(), ra) and torch.equal(gb.cpu(), rb)


# ------------------------------------------------------------------------------------------------------------- merge
@pytest.mark.parametrize("planes,Hs,Ws", SHAPES, ids=IDS)
def test_merge_mean_is_exact_and_spread_is_the_root_of_the_restated_variance(planes, Hs, Ws):
    from m2trans_amd.infer import dihedral_merge
    a, b = _rand(4, planes, Hs, Ws, seed=1 + Hs), _rand(4, planes, Ws, Hs, seed=2 + Ws)
    for t in (a, b):                                             # plane 0: the four corners of all eight outputs equal, so the
        for i in (0, -1):                                        # variance of the four corner pixels is exactly 0
            for j in (0, -1):
                t[:, 0, i, j] = 0.5
    mean_r, var_r, _ = R.merge(a, b)
    assert float(var_r[0, 0, 0, 0]) == 0.0 and float(var_r.max()) > 0.0
    mean, spread = dihedral_merge(a.cuda(), b.cuda(), with_spread=True)
    assert mean.shape == mean_r.shape and spread.shape == mean_r.shape
    assert torch.equal(mean.cpu(), mean_r)
    root = torch.sqrt(var_r)
    assert _within_one_ulp(spread.cpu(), root)
    assert bool((spread.cpu()[var_r == 0] == 0).all())
    only = dihedral_merge(a.cuda(), b.cuda())
    assert torch.equal(only.cpu(), mean_r)


def test_merge_with_a_null_spread_writes_no_spread():
    _lib, lib = _lib_()
    planes, Hs, Ws = 3, 33, 40
    a, b = _rand(4, planes, Hs, Ws, seed=3), _rand(4, planes, Ws, Hs, seed=4)
    n = planes * Hs * Ws
    mbuf, mean = _guarded(n, torch.float32, 7.25)
    sbuf, spread = _guarded(n, torch.float32, -3.5)              # where a spread would go: never passed, stays a canary throughout
    da, db = a.cuda(), b.cuda()
    _lib.check(lib.m2t_dihedral_merge(_lib.ptr(da), _lib.ptr(db), planes, Hs, Ws, _lib.ptr(mean), None, _lib.stream_ptr()), "m2t_dihedral_merge")
    torch.cuda.synchronize()
    assert torch.equal(mean.cpu().view(1, planes, Hs, Ws), R.merge(a, b)[0].view(1, planes, Hs, Ws))
    assert _canaries_hold(mbuf, n, 7.25) and bool((sbuf == -3.5).all())


# ------------------------------------------------------------------------------------------------------------- determinism, canaries
def test_two_runs_are_bit_identical_and_only_the_destinations_are_written():
    _lib, lib = _lib_()
    st = _lib.stream_ptr()
    planes, H, W = 3, 33, 70
    x = _rand(planes, H, W, seed=9)
    n = planes * H * W
    a, b = _rand(4, planes, H, W, seed=10), _rand(4, planes, W, H, seed=11)
    img = _rand(3, H, W, seed=12) * 0.5 + 0.5
    runs = []
    for fill in (7.25, -1.5):
        xb, xs = _guarded(n, torch.float32, fill)
        xs.copy_(x.view(-1))
        ab, av = _guarded(4 * n, torch.float32, fill)
        bb, bv = _guarded(4 * n, torch.float32, fill)
        _lib.check(lib.m2t_dihedral_pack(_lib.ptr(xs), planes, H, W, _lib.ptr(av), _lib.ptr(bv), st), "m2t_dihedral_pack")
        sab, sa = _guarded(4 * n, torch.float32, fill)
        sbb, sb = _guarded(4 * n, torch.float32, fill)
        sa.copy_(a.view(-1))
        sb.copy_(b.view(-1))
        mb, mv = _guarded(n, torch.float32, fill)
        pb, pv = _guarded(n, torch.float32, fill)
        _lib.check(lib.m2t_dihedral_merge(_lib.ptr(sa), _lib.ptr(sb), planes, H, W, _lib.ptr(mv), _lib.ptr(pv), st), "m2t_dihedral_merge")
        ib, iv = _guarded(n, torch.float32, fill)
        iv.copy_(img.view(-1))
        ub, uv = _guarded(n, torch.uint8, 0xA5 if fill > 0 else 0x5A)
        _lib.check(lib.m2t_tensor_to_image_u8(_lib.ptr(iv), 3, H, W, 1.0, _lib.ptr(uv), st), "m2t_tensor_to_image_u8")
        torch.cuda.synchronize()
        for buf, k in ((xb, n), (ab, 4 * n), (bb, 4 * n), (sab, 4 * n), (sbb, 4 * n), (mb, n), (pb, n), (ib, n)):
            assert _canaries_hold(buf, k, fill)
        assert _canaries_hold(ub, n, 0xA5 if fill > 0 else 0x5A)
        assert torch.equal(xs.cpu(), x.view(-1)) and torch.equal(sa.cpu(), a.view(-1)) and torch.equal(sb.cpu(), b.view(-1))
        assert torch.equal(iv.cpu(), img.view(-1))
        runs.append([t.cpu().clone() for t in (av, bv, mv, pv, uv)])
    for first, second in zip(*runs):
        assert torch.equal(first, second)
    wa, wb = R.pack(x[None])
    mean_r, var_r, _ = R.merge(a, b)
    assert torch.equal(runs[0][0], wa.view(-1)) and torch.equal(runs[0][1], wb.view(-1))
    assert torch.equal(runs[0][2], mean_r.view(-1)) and _within_one_ulp(runs[0][3], torch.sqrt(var_r).view(-1))
    assert torch.equal(runs[0][4].view(H, W, 3), R.export_u8(img))


# ------------------------------------------------------------------------------------------------------------- error paths
def test_every_argument_error_is_raised_before_any_launch():
    _lib, lib = _lib_()
    st = _lib.stream_ptr()
    src = torch.zeros(4096, dtype=torch.float32, device="cuda")
    dst = torch.full((4096,), 7.0, dtype=torch.float32, device="cuda")
    d8 = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    s, d, u = _lib.ptr(src), _lib.ptr(dst), _lib.ptr(d8)
    pack_calls = {
        "null src": (None, 3, 8, 8, d, d), "null dst_a": (s, 3, 8, 8, None, d), "null dst_b": (s, 3, 8, 8, d, None),
        "planes 0": (s, 0, 8, 8, d, d), "planes -1": (s, -1, 8, 8, d, d), "planes 65536": (s, 65536, 8, 8, d, d),
        "H 0": (s, 3, 0, 8, d, d), "W 0": (s, 3, 8, 0, d, d), "H -2": (s, 3, -2, 8, d, d),
        "H 16385": (s, 1, 16385, 1, d, d), "W 16385": (s, 1, 1, 16385, d, d),
    }
    for what, a in pack_calls.items():
        assert lib.m2t_dihedral_pack(*a, st) == ARG, what
        with pytest.raises(_lib.M2TError):
            _lib.check(lib.m2t_dihedral_pack(*a, st), what)
    merge_calls = {
        "null sr_a": (None, s, 3, 8, 8, d, d), "null sr_b": (s, None, 3, 8, 8, d, d), "null mean": (s, s, 3, 8, 8, None, d),
        "planes 0": (s, s, 0, 8, 8, d, d), "planes 65536": (s, s, 65536, 8, 8, d, None),
        "Hs 0": (s, s, 3, 0, 8, d, d), "Ws 0": (s, s, 3, 8, 0, d, None), "Hs 16385": (s, s, 1, 16385, 1, d, d), "Ws 16385": (s, s, 1, 1, 16385, d, d),
    }
    for what, a in merge_calls.items():
        assert lib.m2t_dihedral_merge(*a, st) == ARG, what
        with pytest.raises(_lib.M2TError):
            _lib.check(lib.m2t_dihedral_merge(*a, st), what)
    u8_calls = {
        "null src": (None, 3, 8, 8, 1.0, u), "null dst": (s, 3, 8, 8, 1.0, None),
        "channels 0": (s, 0, 8, 8, 1.0, u), "channels 2": (s, 2, 8, 8, 1.0, u), "channels 4": (s, 4, 8, 8, 1.0, u),
        "H 0": (s, 3, 0, 8, 1.0, u), "W 0": (s, 3, 8, 0, 1.0, u), "H 16385": (s, 1, 16385, 1, 1.0, u), "W 16385": (s, 1, 1, 16385, 1.0, u),
        "rgb_range 0": (s, 3, 8, 8, 0.0, u), "rgb_range -1": (s, 3, 8, 8, -1.0, u), "rgb_range inf": (s, 3, 8, 8, float("inf"), u),
        "rgb_range nan": (s, 3, 8, 8, float("nan"), u),
    }
    for what, a in u8_calls.items():
        assert lib.m2t_tensor_to_image_u8(*a, st) == ARG, what
        with pytest.raises(_lib.M2TError):
            _lib.check(lib.m2t_tensor_to_image_u8(*a, st), what)
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((d8 == 0xA5).all())
    # the wrappers raise the same way
    from m2trans_amd import infer
    x = torch.zeros(1, 3, 8, 8, device="cuda")
    bad = [lambda: infer.dihedral_pack(x.double()), lambda: infer.dihedral_pack(x[0]), lambda: infer.dihedral_pack(x[:, :, :, ::2]),
           lambda: infer.dihedral_merge(x.repeat(4, 1, 1, 1), x.repeat(4, 1, 2, 1)), lambda: infer.dihedral_merge(x.repeat(3, 1, 1, 1), x.repeat(3, 1, 1, 1)),
           lambda: infer.self_ensemble(R.nearest_up(2), x.clone().requires_grad_(True)), lambda: infer.self_ensemble(R.nearest_up(2), x[:, :2].contiguous()),
           lambda: infer.self_ensemble(lambda t: t.double(), x), lambda: infer.self_ensemble(lambda t: t[:, :, :, :4], x),
           lambda: infer.to_uint8(x, rgb_range=0.0), lambda: infer.to_uint8(x[:, :2]), lambda: infer.to_uint8(x.cpu())]
    for call in bad:
        with pytest.raises(infer.M2TError):
            call()
    # a second output of another scale than the first
    ups = iter([R.nearest_up(2), R.nearest_up(3)])
    with pytest.raises(infer.M2TError):
        infer.self_ensemble(lambda t: next(ups)(t), torch.zeros(1, 3, 8, 12, device="cuda"))


# ------------------------------------------------------------------------------------------------------------- equivariant stub
@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("shape", [(2, 3, 17, 40), (1, 3, 32, 32)], ids=["2x3x17x40", "1x3x32x32"])
def test_self_ensemble_of_the_equivariant_stub_is_the_stub_itself(s, shape):
    """Nearest-neighbour upsampling commutes with every flip and with the transpose, so all eight U_k are the stub's own output:
    the mean is that output bit for bit and the spread is exactly 0.  A wrong inverse cannot pass."""
    from m2trans_amd.infer import SelfEnsemble, self_ensemble
    x = _rand(*shape, seed=s).cuda()
    up = R.nearest_up(s)
    sr, spread = self_ensemble(up, x, with_spread=True)
    assert torch.equal(sr, up(x)) and torch.equal(spread, torch.zeros_like(spread))
    assert torch.equal(self_ensemble(up, x), sr) and torch.equal(SelfEnsemble(up)(x), sr)
    got = SelfEnsemble(up, with_spread=True)(x)
    assert isinstance(got, tuple) and torch.equal(got[0], sr) and torch.equal(got[1], spread)


# ------------------------------------------------------------------------------------------------------------- the real model
class _Counting:
    def __init__(self, model):
        self.model, self.shapes = model, []

    def __call__(self, x):
        self.shapes.append(tuple(x.shape))
        return self.model(x)


_MODELS = {}


def _model(scale, dtype):
    """M2Trans, n_blocks = 1, random init (seeded); built once per (scale, dtype) and never modified."""
    if (scale, dtype) not in _MODELS:
        from m2trans_amd.M2Trans_network import create_model
        from tests.gpu_util import make_args
        torch.manual_seed(1234 + scale)
        _MODELS[(scale, dtype)] = create_model(make_args(scale, 1, dtype)).to("cuda").eval()
    return _MODELS[(scale, dtype)]


@pytest.mark.parametrize("scale,shape,dtype", [(2, (1, 3, 17, 40), "fp32"), (4, (2, 3, 32, 32), "bf16")], ids=["x2-fp32-17x40", "x4-bf16-32x32"])
def test_self_ensemble_of_the_model_is_the_restatement_on_the_same_batches(scale, shape, dtype):
    from m2trans_amd.infer import self_ensemble
    model = _Counting(_model(scale, dtype))
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(scale)).cuda()
    sr, spread = self_ensemble(model, x, with_spread=True)
    B, _, H, W = shape
    assert model.shapes == ([(8 * B, 3, H, H)] if H == W else [(4 * B, 3, H, W), (4 * B, 3, W, H)])
    with torch.no_grad():
        mean_r, var_r, _ = R.ensemble(model.model, x)            # the same batches built with torch ops, merged in torch
        plain = model.model(x)
    assert bool(torch.isfinite(sr).all()) and tuple(sr.shape) == (B, 3, H * scale, W * scale)
    assert torch.equal(sr, mean_r)
    assert _within_one_ulp(spread.cpu(), torch.sqrt(var_r.cpu()))
    assert not torch.equal(sr, plain) and float(spread.max()) > 0.0


# ------------------------------------------------------------------------------------------------------------- export
@pytest.mark.parametrize("rgb_range", [1.0, 255.0])
def test_to_uint8_equals_the_torch_expression(rgb_range, tmp_path):
    from m2trans_amd.infer import save_image, to_uint8
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(int(rgb_range))
    for C, H, W in ((3, 17, 40), (3, 5, 7), (1, 9, 13), (1, 8, 8), (3, 33, 64)):     # H W a multiple of 4 or not, with a tail
        x = (torch.rand(C, H, W, generator=g) * 1.4 - 0.2) * rgb_range               # below 0 and above the range
        flat = x.view(-1)
        k = torch.arange(flat.numel() // 2, dtype=torch.float32) % 256
        flat[::2][:k.numel()] = (k + 0.5) * (rgb_range / 255.0)                     # .5 ties (exact for rgb_range 255), 255.5 included
        flat[1], flat[3] = -0.1 * rgb_range, 1.3 * rgb_range
        assert float(x.min()) < 0 and float(x.max()) > rgb_range
        want = R.export_u8(x, rgb_range)
        got = to_uint8(x.cuda(), rgb_range)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W, C) and torch.equal(got.cpu(), want)
        assert torch.equal(to_uint8(x[None].cuda(), rgb_range).cpu(), want)
        # unaligned bases: the source one float and the destination one byte off (no 16-byte loads, no dword stores)
        src = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")[1:]
        src.copy_(flat)
        dbuf, dst = _guarded(x.numel(), torch.uint8, 0xA5)
        _lib.check(lib.m2t_tensor_to_image_u8(_lib.ptr(src), C, H, W, rgb_range, _lib.ptr(dst), _lib.stream_ptr()), "m2t_tensor_to_image_u8")
        assert torch.equal(dst.cpu().view(H, W, C), want) and _canaries_hold(dbuf, x.numel(), 0xA5)
    if rgb_range == 255.0:
        ties = torch.tensor([0.5, 1.5, 127.5, 254.5, 255.5, -0.5]).view(1, 1, 6)
        assert to_uint8(ties.cuda(), 255.0).view(-1).tolist() == [1, 2, 128, 255, 255, 0]
    # through a file: PIL reads back the same array
    from PIL import Image
    rgb = torch.rand(3, 24, 40, generator=g) * rgb_range
    save_image(rgb[None].cuda(), tmp_path / "rgb.png", rgb_range)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "rgb.png")), R.export_u8(rgb, rgb_range).numpy())
    save_image(rgb[:1].cuda(), tmp_path / "grey.png", rgb_range)
    back = Image.open(tmp_path / "grey.png")
    assert back.mode == "L" and np.array_equal(np.asarray(back), R.export_u8(rgb[:1], rgb_range).numpy()[:, :, 0])


def test_to_uint8_sends_nan_to_zero():
    from m2trans_amd.infer import to_uint8
    x = torch.full((3, 6, 10), 0.5)
    x[0, 1, 2] = float("nan")
    x[2, 5, 9] = float("nan")
    x[1, 0, 0] = float("inf")
    x[1, 0, 1] = -float("inf")
    got = to_uint8(x.cuda()).cpu()
    assert int(got[1, 2, 0]) == 0 and int(got[5, 9, 2]) == 0 and int(got[0, 0, 1]) == 255 and int(got[0, 1, 1]) == 0
    assert torch.equal(got, R.export_u8(x)) and int((got == 128).sum()) == x.numel() - 4


# ------------------------------------------------------------------------------------------------------------- evaluate, folders
def test_evaluate_with_self_ensemble_wraps_the_model():
    from m2trans_amd.infer import SelfEnsemble
    from m2trans_amd.metrics import evaluate
    scale = 2
    model = _model(scale, "fp32")
    g = torch.Generator().manual_seed(77)
    pairs = [(torch.rand(1, 3, h, w, generator=g).cuda(), torch.rand(1, 3, h * scale, w * scale, generator=g).cuda()) for h, w in ((24, 40), (32, 32))]
    got = evaluate(model, pairs, scale, self_ensemble=True)
    want = evaluate(SelfEnsemble(model), pairs, scale)
    assert got == want and len(got) == 2, (got, want)
    assert evaluate(model, pairs, scale, self_ensemble=False) == evaluate(model, pairs, scale)


def test_upscale_folder_writes_what_to_uint8_of_the_ensemble_gives(tmp_path):
    from PIL import Image
    from m2trans_amd import infer
    scale = 2
    model = _model(scale, "fp32")
    src, out, sp, plain = tmp_path / "lr", tmp_path / "sr", tmp_path / "spread", tmp_path / "plain"
    src.mkdir()
    rng = np.random.default_rng(3)
    sizes = {"b_wide.png": (24, 40), "a_square.png": (32, 32)}
    for name, (h, w) in sizes.items():
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(src / name)
    written = infer.upscale_folder(model, src, out, self_ensemble=True, spread_dir=sp)
    assert written == ["a_square.png", "b_wide.png"]
    factors = json.load(open(sp / "spread.json"))
    assert set(factors["max_spread"]) == set(sizes) and factors["rgb_range"] == 1.0
    for name, (h, w) in sizes.items():
        lr = infer.load_image(src / name, "cuda")
        assert tuple(lr.shape) == (1, 3, h, w)
        sr, spread = infer.self_ensemble(model, lr, with_spread=True)
        img = Image.open(out / name)
        assert img.mode == "RGB" and img.size == (w * scale, h * scale)
        assert np.array_equal(np.asarray(img), infer.to_uint8(sr).cpu().numpy())
        grey = spread[0].amax(dim=0, keepdim=True)
        top = float(grey.max())
        assert top > 0.0 and factors["max_spread"][name] == top
        simg = Image.open(sp / name)
        assert simg.mode == "L" and simg.size == (w * scale, h * scale)
        assert np.array_equal(np.asarray(simg), infer.to_uint8(grey, top).cpu().numpy()[:, :, 0]) and int(np.asarray(simg).max()) == 255
    # without the ensemble: the model's own output, and no spread
    assert infer.upscale_folder(model, src, plain) == written and not os.path.exists(plain / "spread.json")
    lr = infer.load_image(src / "b_wide.png", "cuda")
    with torch.no_grad():
        assert np.array_equal(np.asarray(Image.open(plain / "b_wide.png")), infer.to_uint8(model(lr)).cpu().numpy())
    with pytest.raises(infer.M2TError):
        infer.upscale_folder(model, src, plain, spread_dir=sp)   # a spread needs the ensemble


@pytest.mark.parametrize("form", ["checkpoint", "state_dict_with_module_prefix"])
def test_the_command_line_loads_a_checkpoint_and_writes_the_models_output(tmp_path, form, capsys):
    """`python -m m2trans_amd.infer` in process (its `main`): yaml -> create_model, the weights from a train.py-style checkpoint or a
    bare state_dict with DataParallel's prefix, one image in, the model's own output out."""
    import yaml
    from PIL import Image
    from m2trans_amd import infer
    scale = 2
    model = _model(scale, "fp32")
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    if form == "checkpoint":
        torch.save({"epoch": 3, "model_state_dict": sd}, tmp_path / "m.pt")
    else:
        torch.save({"module." + k: v for k, v in sd.items()}, tmp_path / "m.pt")
    with open(tmp_path / "c.yml", "w") as f:
        yaml.safe_dump({"model": "M2Trans", "scale": scale, "n_blocks": 1, "n_feats": 64, "colors": 3, "rgb_range": 1.0, "compute_dtype": "bf16"}, f)
    (tmp_path / "in").mkdir()
    Image.fromarray(np.random.default_rng(5).integers(0, 256, size=(24, 40, 3), dtype=np.uint8)).save(tmp_path / "in" / "img.png")
    argv = ["--config", str(tmp_path / "c.yml"), "--model_path", str(tmp_path / "m.pt"), "--input", str(tmp_path / "in"),
            "--output", str(tmp_path / "out"), "--compute_dtype", "fp32"]
    assert infer.main(argv) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["images"] == 1
    lr = infer.load_image(tmp_path / "in" / "img.png", "cuda")
    with torch.no_grad():
        want = infer.to_uint8(model(lr)).cpu().numpy()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "img.png")), want)
    assert infer.main(argv + ["--self_ensemble", "--spread", str(tmp_path / "sp")]) == 0
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "img.png")), infer.to_uint8(infer.self_ensemble(model, lr)).cpu().numpy())
    assert os.path.exists(tmp_path / "sp" / "img.png") and os.path.exists(tmp_path / "sp" / "spread.json")
