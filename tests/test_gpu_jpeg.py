"""GPU tests of the JPEG stage (include/m2t_jpeg.h, k_jpeg.hip, m2trans_amd/degrade.py): every output of m2t_degrade_jpeg_patches,
m2t_degrade_jpeg_image_u8 and m2t_jpeg_image_u8 against the NumPy fp64 restatements (tests/degrade_ref.py, then tests/jpeg_ref.py, then
the flips) on every bit -- no tolerance anywhere -- the skip path against m2t_degrade_patches, locality, determinism, the argument
errors, the datasets, the resumed run and the tool."""
import copy
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from tests import degrade_ref as R
from tests import jpeg_ref as J

pytestmark = pytest.mark.gpu

SEED = (5 << 32) + 33
QUALITIES = (1, 10, 50, 95, 100)


@pytest.fixture(scope="module")
def consts():
    from m2trans_amd.degrade import jpeg_constants
    c = jpeg_constants()
    return c[:64].reshape(8, 8).copy(), c[64:].copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _descriptors(hr_images, items, gray, cols):
    """items: (image, lx, ly, flags, bank index, sigma_add, sigma_speckle, noise_id[, quality]) -> (pool, desc [n, cols])."""
    offs = np.cumsum([0] + [im.size for im in hr_images])
    pool = torch.from_numpy(np.concatenate([im.reshape(-1) for im in hr_images])).cuda()
    desc = np.zeros((len(items), cols), dtype=np.int64)
    lev = np.zeros((len(items), 2))
    for k, it in enumerate(items):
        img, lx, ly, flags, index, sa, ss, nid = it[:8]
        H, W, _ = hr_images[img].shape
        desc[k, :8] = (offs[img], H, W, lx, ly, flags, index, nid - (1 << 64) if nid >= 1 << 63 else nid)
        lev[k] = (sa, ss)
        desc[k, 10] = int(gray)
        if cols > 11:
            desc[k, 11] = it[8]
    desc[:, 8:10] = lev.view(np.int64)
    return pool, desc


def _call_jpeg_patches(hr_images, kernels, s, lp, items, gray, seed=SEED, K=None, M=None, prefill=None, desc_edit=None, patch_size=None,
                       channels=3, no_consts=False):
    """m2t_degrade_jpeg_patches on a pool of `hr_images` -> (rc, lr, hr) on the host."""
    from m2trans_amd import _lib
    from m2trans_amd.degrade import _jpeg_constants_on
    lib = _lib.load()
    pool, desc = _descriptors(hr_images, items, gray, _lib.JPEG_DESC_COLS)
    bank = torch.from_numpy(np.ascontiguousarray(kernels, dtype=np.float64)).cuda()
    if desc_edit is not None:
        desc_edit(desc)
    n = len(items)
    fill = float("nan") if prefill is None else prefill
    lr = torch.full((n, 3, lp, lp), fill, dtype=torch.float32, device="cuda")
    hr = torch.full((n, 3, lp * s, lp * s), fill, dtype=torch.float32, device="cuda")
    rc = lib.m2t_degrade_jpeg_patches(_lib.ptr(pool), _lib.ptr(bank), kernels.shape[0] if M is None else M, kernels.shape[1] if K is None else K,
                                      None if no_consts else _lib.ptr(_jpeg_constants_on("cuda")), desc.ctypes.data_as(C.c_void_p), n, channels,
                                      lp * s if patch_size is None else patch_size, s, seed, _lib.ptr(lr), _lib.ptr(hr), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, lr.cpu().numpy(), hr.cpu().numpy()


def _call_plain_patches(hr_images, kernels, s, lp, items, gray, seed=SEED):
    from m2trans_amd import _lib
    lib = _lib.load()
    pool, desc = _descriptors(hr_images, items, gray, _lib.DEGRADE_DESC_COLS)
    bank = torch.from_numpy(np.ascontiguousarray(kernels, dtype=np.float64)).cuda()
    n = len(items)
    lr = torch.full((n, 3, lp, lp), float("nan"), dtype=torch.float32, device="cuda")
    hr = torch.full((n, 3, lp * s, lp * s), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.m2t_degrade_patches(_lib.ptr(pool), _lib.ptr(bank), kernels.shape[0], kernels.shape[1], desc.ctypes.data_as(C.c_void_p), n, 3,
                                 lp * s, s, seed, _lib.ptr(lr), _lib.ptr(hr), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, lr.cpu().numpy(), hr.cpu().numpy()


def _image(H, W, seed, colour=True):
    rng = np.random.RandomState(seed)
    if colour:
        return rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(rng.randint(0, 256, size=(H, W, 1)).astype(np.uint8), 3, axis=2))


def _items(s, K, lp, n, far):
    """n items: the two images in turn, both corners, every flag value, both noises on (a few with one or none), the five
    qualities in turn and one item of quality 0 in the middle."""
    levels = [(6.0, 0.2)] * 5 + [(0.0, 0.0), (6.0, 0.0), (0.0, 0.2)]
    out = []
    for k in range(n):
        lx, ly = far if (k // 8) % 2 else (0, 0)
        sa, ss = levels[(k // 3) % 8]
        quality = 0 if k == 7 else QUALITIES[k % 5]
        out.append((k % 2, lx, ly, k % 8, k % 3, sa, ss, (k * 0x9E3779B97F4A7C15 + K) & ((1 << 64) - 1), quality))
    return out


# ------------------------------------------------------------------------------------------------------------- patches
@pytest.mark.parametrize("lp", [8, 16, 24, 40])
@pytest.mark.parametrize("s,K", [(2, 2), (2, 20), (3, 1), (3, 21), (4, 2), (4, 20)])
def test_patches_equal_the_restatements_on_every_bit(consts, s, K, lp):
    """degrade -> jpeg -> flips, 33 items per call (two by-value chunks): lp = 8 is one block of a tile, 16 one tile, 24 and 40 several
    tiles with partial ones (a half and a quarter of their blocks absent); a grey and a colour HR image, the corner (0, 0) and the
    largest one, all 8 flag values, qualities 1, 10, 50, 95, 100 and one item of quality 0; gray noise on (small K) and off."""
    T, recip = consts
    H, W = (lp + 3) * s + 1, (lp + 5) * s
    images = [_image(H, W, 10 * s + lp, colour=False), _image(H, W, 11 * s + lp, colour=True)]
    kernels = R.bank(s, M=3, K=K, seed=11)[0]
    gray = K <= 2
    items = _items(s, K, lp, 33, (W // s - lp, H // s - lp))
    rc, lr, hr = _call_jpeg_patches(images, kernels, s, lp, items, gray)
    assert rc == 0
    want_lr, want_hr = J.patches(images, kernels, s, lp, items, T, recip, gray, SEED)
    bad = np.argwhere(_bits(lr) != _bits(want_lr))
    assert bad.size == 0, (len(bad), bad[:4].tolist(), items[bad[0][0]])
    assert np.array_equal(_bits(hr), _bits(want_hr))                                 # the HR half: the restatement of m2t_crop_patches
    plain_lr, _ = R.patches(images, kernels, s, lp, [it[:8] for it in items], gray, SEED)
    assert np.array_equal(_bits(lr[7]), _bits(plain_lr[7]))                          # quality 0 inside the batch
    assert not np.array_equal(lr[0], plain_lr[0])                                    # quality 1 is not a no-op


def test_every_quality_zero_gives_the_bytes_of_degrade_patches():
    s, K, lp = 4, 12, 24
    images = [_image(120, 130, 1, colour=False), _image(120, 130, 2)]
    kernels = R.bank(s, M=3, K=K, seed=5)[0]
    items = [it[:8] + (0,) for it in _items(s, K, lp, 33, (130 // s - lp, 120 // s - lp))]
    for gray in (True, False):
        rc, lr, hr = _call_jpeg_patches(images, kernels, s, lp, items, gray)
        rc0, lr0, hr0 = _call_plain_patches(images, kernels, s, lp, [it[:8] for it in items], gray)
        assert rc == rc0 == 0 and np.array_equal(_bits(lr), _bits(lr0)) and np.array_equal(_bits(hr), _bits(hr0))


# ------------------------------------------------------------------------------------------------------------- whole images
@pytest.mark.parametrize("lh,lw", [(13, 19), (33, 17), (1, 1), (8, 8)])
def test_whole_images_equal_the_restatement_on_every_byte(consts, lh, lw):
    from m2trans_amd.degrade import Degradation, jpeg_roundtrip
    T, recip = consts
    for colour in (False, True):
        img = _image(lh, lw, lh * 7 + lw, colour)
        dev = torch.from_numpy(img).cuda()
        for quality in QUALITIES:
            got = jpeg_roundtrip(dev, quality).cpu().numpy()
            assert np.array_equal(got, J.roundtrip(img, quality, T, recip)), (colour, quality)
        assert np.array_equal(dev.cpu().numpy(), img)                                # the input is left alone
    for s, extra in ((2, (1, 0)), (3, (2, 1)), (4, (0, 3))):
        hr = _image(lh * s + extra[0], lw * s + extra[1], lh + s)
        dev = torch.from_numpy(hr).cuda()
        for gray in (True, False):
            D = Degradation(s, bank=4, seed=SEED, gray_noise=gray)
            for index, sa, ss, nid, quality in ((0, 0.0, 0.0, 0, 50), (3, 4.0, 0.15, (1 << 63) + 9, 10), (2, 7.0, 0.0, 5, 95), (1, 3.0, 0.1, 6, 0)):
                got = D.apply_image(dev, index=index, sigma_add=sa, sigma_speckle=ss, noise_id=nid, quality=quality).cpu().numpy()
                want = J.image_u8(hr, D.kernels[index], s, T, recip, quality, sa, ss, gray, nid, SEED)
                assert got.shape == (lh, lw, 3) and np.array_equal(got, want), (s, gray, quality, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------------------- robustness
def test_locality_determinism_and_full_overwrite(consts):
    from m2trans_amd.degrade import jpeg_roundtrip
    img = _image(40, 56, 3)
    dev = torch.from_numpy(img).cuda()
    base = jpeg_roundtrip(dev, 50)
    poked = img.copy()
    poked[19, 41] = 255 - poked[19, 41]                                              # block row 2, block column 5: the second tile column
    diff = np.argwhere((jpeg_roundtrip(torch.from_numpy(poked).cuda(), 50) != base).any(dim=2).cpu().numpy())
    assert len(diff) > 1 and (diff[:, 0] // 8 == 2).all() and (diff[:, 1] // 8 == 5).all()
    for poison in (0, 171, 255):
        out = torch.full_like(dev, poison)
        assert jpeg_roundtrip(dev, 50, out=out) is out and torch.equal(out, base)
    images = [_image(60, 64, 4)]
    kernels = R.bank(2, M=2, K=8, seed=2)[0]
    items = [(0, k % 5, k % 3, k % 8, k % 2, 5.0, 0.1, 100 + k, QUALITIES[k % 5]) for k in range(33)]
    rc, lr1, hr1 = _call_jpeg_patches(images, kernels, 2, 24, items, True)
    rc2, lr2, hr2 = _call_jpeg_patches(images, kernels, 2, 24, items, True, prefill=-3.0)
    assert rc == rc2 == 0 and np.array_equal(_bits(lr1), _bits(lr2)) and np.array_equal(_bits(hr1), _bits(hr2))
    assert np.isfinite(lr1).all() and np.isfinite(hr1).all()                         # the NaN prefill is gone


# ------------------------------------------------------------------------------------------------------------- argument errors
def _set(col, value, row=1):
    def edit(desc):
        desc[row, col] = value
    return edit


def test_argument_errors_come_before_any_launch():
    from m2trans_amd import _lib
    from m2trans_amd._lib import M2TError
    from m2trans_amd.degrade import Degradation, _jpeg_constants_on, jpeg_roundtrip
    lib = _lib.load()
    images = [_image(36, 40, 4)]
    k2 = R.bank(2, M=2, K=8, seed=2)[0]
    items = [(0, 1, 2, 3, 1, 5.0, 0.1, 9, 50)] * 3

    def refused(what, s=2, **kw):
        rc, lr, hr = _call_jpeg_patches(images, k2, s, 8, items, True, **kw)
        assert rc == -2, (what, rc)
        assert np.isnan(lr).all() and np.isnan(hr).all(), what                       # nothing was launched
        return lib.m2t_last_error_string().decode()

    assert "quality" in refused("quality 101", desc_edit=_set(11, 101))
    assert "quality" in refused("quality -1", desc_edit=_set(11, -1))
    assert "quality" in refused("quality 101, last item", desc_edit=_set(11, 101, row=2))
    assert "m2t_degrade_jpeg_patches" in refused("no constants", no_consts=True)
    # what m2t_degrade_patches refuses
    assert "scale" in refused("scale 5", s=5)
    assert "parity" in refused("odd K at x2", K=7)
    assert "empty" in refused("M 0", M=0)
    assert "bank index" in refused("bank index M", desc_edit=_set(6, 2))
    assert "outside the image" in refused("lx beyond", desc_edit=_set(3, 13))
    assert "out of range" in refused("lx < 0", desc_edit=_set(3, -1))
    assert "flags" in refused("flags 8", desc_edit=_set(5, 8))
    assert "level" in refused("level -1", desc_edit=lambda d: d.__setitem__((1, 8), np.array([-1.0]).view(np.int64)[0]))
    assert "gray" in refused("gray 2", desc_edit=_set(10, 2))
    assert "multiple" in refused("patch 15", patch_size=15)
    assert "3 channels" in refused("one channel", channels=1)
    # the image entries
    D = Degradation(2, kernels=k2, seed=3)
    dev = torch.from_numpy(images[0]).cuda()
    out = torch.full((18, 20, 3), 171, dtype=torch.uint8, device="cuda")
    for kw in (dict(quality=101), dict(quality=-1), dict(quality=50, index=2), dict(quality=50, sigma_add=-1.0)):
        with pytest.raises(M2TError, match="m2t_degrade_jpeg_image_u8"):
            D.apply_image(dev, out=out, **kw)
    with pytest.raises(M2TError, match="quality"):
        D.apply_image(dev, out=out, quality=50.0)
    same = torch.full_like(dev, 171)
    for q in (0, 101, -5, 50.0, True):
        with pytest.raises(M2TError, match="quality"):
            jpeg_roundtrip(dev, q, out=same)
    with pytest.raises(M2TError, match="uint8"):
        jpeg_roundtrip(dev.float(), 50)
    with pytest.raises(M2TError, match="out must be"):
        jpeg_roundtrip(dev, 50, out=dev)
    torch.cuda.synchronize()
    assert bool((out == 171).all()) and bool((same == 171).all())
    one, cst = C.c_void_p(8), _lib.ptr(_jpeg_constants_on("cuda"))
    assert lib.m2t_jpeg_image_u8(one, 4, 4, 3, cst, 0, one, None) == -2
    assert "quality" in lib.m2t_last_error_string().decode()
    assert lib.m2t_jpeg_image_u8(one, 4, 4, 3, cst, 101, one, None) == -2
    assert lib.m2t_jpeg_image_u8(one, 0, 4, 3, cst, 50, one, None) == -2
    assert lib.m2t_jpeg_image_u8(one, 4, 4, 1, cst, 50, one, None) == -2
    assert lib.m2t_jpeg_image_u8(one, 4, 4, 3, None, 50, one, None) == -2
    assert lib.m2t_jpeg_image_u8(None, 4, 4, 3, cst, 50, one, None) == -2
    assert lib.m2t_degrade_jpeg_image_u8(one, 36, 40, 3, one, 2, 8, 0, 2, 0, 0, 0.0, 0.0, 1, None, 50, one, None) == -2
    assert lib.m2t_degrade_jpeg_image_u8(one, 36, 40, 3, one, 2, 8, 0, 2, 0, 0, 0.0, 0.0, 1, cst, 101, one, None) == -2
    assert lib.m2t_degrade_jpeg_image_u8(one, 36, 40, 3, one, 2, 7, 0, 2, 0, 0, 0.0, 0.0, 1, cst, 50, one, None) == -2
    assert lib.m2t_degrade_jpeg_image_u8(one, 1, 40, 3, one, 2, 8, 0, 2, 0, 0, 0.0, 0.0, 1, cst, 50, one, None) == -2


# ------------------------------------------------------------------------------------------------------------- datasets
def _train_images():
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:96, 0:112]
    out = []
    for k in range(3):
        base = 120 + 80 * np.sin(xx / (7.0 + k) + k) * np.cos(yy / (11.0 - k))
        img = np.stack([base, base, base], axis=2) + rng.randint(0, 30, size=(96, 112, 1))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def test_us1k_batch_equals_the_restatement_driven_by_a_copy(consts):
    from m2trans_amd.datas import US1K
    from m2trans_amd.degrade import Degradation
    T, recip = consts
    imgs = _train_images()
    D = Degradation(4, bank=8, ksize=10, noise=(1.0, 9.0), speckle=(0.0, 0.2), seed=SEED, jpeg=(30, 95), jpeg_prob=0.7)
    twin = copy.deepcopy(D)
    ds = US1K(images=[(im, None) for im in imgs], scale=4, patch_size=64, repeat=3, device="cuda", degradation=D)
    plain = US1K(images=[(im, None) for im in imgs], scale=4, patch_size=64, repeat=3, device="cuda")
    idx = [4, 0, 5, 2, 1, 8, 7]
    random.seed(7)
    lr, hr = ds.batch(idx)
    after = random.getstate()
    random.seed(7)
    items = []
    for i in idx:
        lx, ly, flags = plain.draw(i)
        items.append((i % 3, lx, ly, flags) + twin.draw() + (twin.draw_jpeg(),))
    assert random.getstate() == after                             # the degradation draws nothing from the global generator
    qs = [it[8] for it in items]
    assert 0 in qs and any(q > 0 for q in qs)                     # jpeg_prob = 0.7: both kinds in this batch
    want_lr, want_hr = J.patches(imgs, twin.kernels, 4, 16, items, T, recip, True, SEED)
    assert np.array_equal(_bits(lr.cpu().numpy()), _bits(want_lr)) and np.array_equal(_bits(hr.cpu().numpy()), _bits(want_hr))
    assert D.get_state() == twin.get_state() and D.draw()[3] == 7
    # without `jpeg` the dataset holds no constants and its batch is the one of m2t_degrade_patches
    E = Degradation(4, bank=8, ksize=10, noise=(1.0, 9.0), speckle=(0.0, 0.2), seed=SEED)
    twin = copy.deepcopy(E)
    off = US1K(images=[(im, None) for im in imgs], scale=4, patch_size=64, repeat=3, device="cuda", degradation=E)
    assert off._jpeg is None and ds._jpeg is not None
    random.seed(7)
    lr_off, _ = off.batch(idx)
    random.seed(7)
    items = [(i % 3,) + plain.draw(i) + twin.draw() for i in idx]
    assert np.array_equal(_bits(lr_off.cpu().numpy()), _bits(R.patches(imgs, twin.kernels, 4, 16, items, True, SEED)[0]))


def test_benchmark_is_the_same_at_every_construction(consts):
    from m2trans_amd.datas import Benchmark
    from m2trans_amd.degrade import BENCHMARK_NOISE_ID, Degradation
    T, recip = consts
    imgs = _train_images()
    D = Degradation(4, bank=8, ksize=10, noise=(1.0, 9.0), speckle=(0.0, 0.2), seed=SEED, jpeg=(30, 95))
    state = D.get_state()
    entries = [(imgs[0][:50, :67].copy(), None, "a.png"), (imgs[1], None, "b.png")]
    a = Benchmark(images=entries, scale=4, device="cuda", degradation=D)
    b = Benchmark(images=entries, scale=4, device="cuda", degradation=D)
    assert D.get_state() == state                                 # validation does not advance the training draws
    rng = random.Random(SEED)
    for k, ((la, ha, na), (lb, hb, nb)) in enumerate(zip(a, b)):
        assert na == nb and torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(ha, hb)
        hr = entries[k][0]
        hr = hr[:hr.shape[0] // 4 * 4, :hr.shape[1] // 4 * 4]
        index, sa, ss = D.draw_levels(rng)
        quality = D.draw_jpeg(rng)                                # right after draw_levels, on the same generator
        assert 30 <= quality <= 95
        want = J.image_u8(hr, D.kernels[index], 4, T, recip, quality, sa, ss, True, BENCHMARK_NOISE_ID + k, SEED)
        assert np.array_equal(_bits(la[0].cpu().numpy()), _bits(R.to_tensor(want)))


# ------------------------------------------------------------------------------------------------------------- resume
def _fit(out_dir, **kw):
    from m2trans_amd import train as T
    from m2trans_amd.datas import US1K, Benchmark
    from m2trans_amd.degrade import Degradation
    from m2trans_amd.train_step import TrainStep
    from tests.gpu_util import build_model
    model, _ = build_model(2, 1, "fp32")
    ts = TrainStep(model, lr=2e-4, world_size=1)
    imgs = _train_images()
    D = Degradation(2, bank=8, noise=(1.0, 9.0), speckle=(0.0, 0.2), seed=SEED, jpeg=(30, 95), jpeg_prob=0.8)
    ds = US1K(images=[(im, None) for im in imgs], scale=2, patch_size=64, repeat=2, device="cuda", degradation=D)
    valid = [("mine", Benchmark(images=[(imgs[0][:64, :64].copy(), None, "a.png")], scale=2, device="cuda", degradation=D))]
    lines = []
    args = dict(epochs=2, batch_size=2, lr0=2e-4, eta_min=1e-6, log_every=1, test_every=1, out_dir=str(out_dir), patch_size=64,
                preview_every=100, seed=33, ring_rows=8, log=lines.append)
    args.update(kw)
    stat = T.fit(model, ts, ds, valid, **args)
    torch.cuda.synchronize()
    return {"params": model.flat_params.detach().cpu().clone(), "exp_avg": ts.exp_avg.cpu().clone(), "exp_avg_sq": ts.exp_avg_sq.cpu().clone(),
            "steps": ts.step_count, "stat": stat, "lines": lines, "D": D}


def test_resume_with_jpeg_repeats_the_uninterrupted_run(tmp_path):
    full = _fit(tmp_path / "full")
    assert full["steps"] == 6 and full["D"].get_state()["noise_id"] == 12
    ckpt = torch.load(tmp_path / "full" / "models" / "model_x2_1.pt", map_location="cpu", weights_only=False)
    assert set(ckpt["m2t_rng"]["degradation"]) == {"random", "noise_id"} and ckpt["m2t_rng"]["degradation"]["noise_id"] == 6
    first = _fit(tmp_path / "cut", last_epoch=1)
    assert first["steps"] == 3
    second = _fit(tmp_path / "cut", resume=str(tmp_path / "cut"))                   # fresh objects: the state comes from the file
    assert second["steps"] == 6 and second["D"].get_state() == full["D"].get_state()
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(second[k], full[k]), k
    assert second["stat"] == full["stat"]
    assert not torch.equal(first["params"], full["params"])


# ------------------------------------------------------------------------------------------------------------- the tool, the yaml key
def test_make_lr_and_the_config_key_reach_the_stage(tmp_path, capsys, consts):
    """tools/make_lr.py --degradation with `jpeg:` in the mapping writes what the restatement computes in sorted file order, and
    train.build_datasets hands the same mapping to the training set, whose batch equals the restatement."""
    import importlib.util
    import json
    import yaml
    from PIL import Image
    from m2trans_amd import train as TR
    from m2trans_amd.degrade import BENCHMARK_NOISE_ID, from_config
    T, recip = consts
    imgs = _train_images()
    hr_dir = tmp_path / "hr"
    hr_dir.mkdir()
    Image.fromarray(imgs[0][:50, :67].copy(), "RGB").save(hr_dir / "b.png")
    Image.fromarray(imgs[1], "RGB").save(hr_dir / "a.png")
    cfg = {"bank": 8, "ksize": 7, "noise": [1.0, 9.0], "speckle": [0.0, 0.2], "seed": 12, "jpeg": [30, 95], "jpeg_prob": 1.0}
    (tmp_path / "deg.yml").write_text(yaml.safe_dump({"degradation": cfg}))
    spec = importlib.util.spec_from_file_location("make_lr_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 "tools", "make_lr.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(["--hr", str(hr_dir), "--out", str(tmp_path / "lr"), "--scale", "3", "--degradation", str(tmp_path / "deg.yml")])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["images"] == 2 and line["degradation"] is True
    D = from_config(3, cfg)
    assert D.jpeg == (30, 95)
    rng = random.Random(12)
    for k, (name, hr) in enumerate((("a", imgs[1]), ("b", imgs[0][:50, :67]))):
        hr = hr[:hr.shape[0] // 3 * 3, :hr.shape[1] // 3 * 3]
        index, sa, ss = D.draw_levels(rng)
        quality = D.draw_jpeg(rng)
        want = J.image_u8(hr, D.kernels[index], 3, T, recip, quality, sa, ss, True, BENCHMARK_NOISE_ID + k, 12)
        got = np.asarray(Image.open(tmp_path / "lr" / "X3" / f"{name}x3.png").convert("RGB"))
        assert np.array_equal(got, want), name
        assert not np.array_equal(want, R.image_u8(hr, D.kernels[index], 3, sa, ss, True, BENCHMARK_NOISE_ID + k, 12))
    # the yaml key of a training config
    (tmp_path / "train").mkdir()
    for k, im in enumerate(imgs):
        Image.fromarray(im, "RGB").save(tmp_path / "train" / f"{k}.png")
    tcfg = {"scale": 2, "patch_size": 64, "batch_size": 2, "epochs": 1, "lr": 1e-4, "eta_min": 1e-6, "log_every": 1, "test_every": 1,
            "training_dataset": "folder", "train_hr_path": str(tmp_path / "train"), "eval_folders": {"mine": str(tmp_path / "val")},
            "degradation": {"bank": 4, "ksize": 6, "noise": [2.0, 2.0], "speckle": [0.0, 0.0], "seed": 21, "jpeg": [40, 60]}}
    (tmp_path / "val").mkdir()
    Image.fromarray(imgs[0][:64, :64].copy(), "RGB").save(tmp_path / "val" / "v.png")
    train, valid = TR.build_datasets(TR.resolve_config(tcfg)["data"])
    assert train.degradation.jpeg == (40, 60) and valid[0][1].degradation is train.degradation
    random.seed(3)
    lr, hr = train.batch([0, 1])
    twin = from_config(2, tcfg["degradation"])
    random.seed(3)
    items = []
    for i in (0, 1):
        lx, ly, flags = train.draw(i)
        items.append((i, lx, ly, flags) + twin.draw() + (twin.draw_jpeg(),))
    want_lr, want_hr = J.patches(imgs, twin.kernels, 2, 32, items, T, recip, True, 21)
    assert np.array_equal(_bits(lr.cpu().numpy()), _bits(want_lr)) and np.array_equal(_bits(hr.cpu().numpy()), _bits(want_hr))
