"""-m gpu: the bicubic resampler (k_resize.hip; m2t_imresize_u8, m2t_imresize_f32, resize.py, the LR synthesis of datas.US1K /
datas.Benchmark, resize.BicubicUp under metrics.evaluate, tools/make_lr.py) against the fp64 restatement tests/imresize_ref.py.

uint8: every pixel equal to the quantised reference.  x2 and x4 are exact in fp64 (weights are multiples of 2^-12), so their ties
are true ties resolved by the rounding rule; x3 leaves about 1e-13 of freedom, and every x3 input is asserted to keep its
pre-rounding values at least 1e-6 from a half-integer (a condition on the inputs, checked on what is actually run).
float32: |dev - ref64| <= 2^-23 |ref64| + 1e-30, one fp32 rounding."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import imresize_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -2
MARGIN = 1e-6
CASES = [(s, up) for s in R.SCALES for up in (False, True)]
IDS = [f"x{s}{'up' if up else 'down'}" for s, up in CASES]


def _lib_():
    from m2trans_amd import _lib
    return _lib, _lib.load()


def _off_ties(s, values):
    if s == 3:
        m = min(R.tie_margin(v) for v in values)
        assert m >= MARGIN, m


# ------------------------------------------------------------------------------------------------------------- uint8
@pytest.mark.parametrize("s,up", CASES, ids=IDS)
def test_imresize_u8_equals_the_quantised_reference_on_every_pixel(s, up):
    from m2trans_amd.resize import imresize_u8
    cases = R.u8_cases(s, up)
    _off_ties(s, [v for _, _, v in cases])
    for name, img, v in cases:
        got = imresize_u8(torch.from_numpy(img).cuda(), s, up=up)
        want = torch.from_numpy(R.quantise(v))
        assert got.shape == want.shape and got.dtype == torch.uint8, (name, got.shape, want.shape)
        bad = int((got.cpu() != want).sum())
        assert bad == 0 and torch.equal(got.cpu(), want), (name, bad)


@pytest.mark.parametrize("s,up", CASES, ids=IDS)
def test_two_runs_are_bit_identical_and_only_the_destination_is_written(s, up):
    """dst sits between guard bytes in one allocation, at an odd offset (packed stores meet an unaligned base), pre-filled with two
    different sentinels: both runs give the reference on every byte (so every byte was written), the guards keep the sentinel."""
    _lib, lib = _lib_()
    name, img, v = R.u8_cases(s, up)[-1]                         # 70 x 131 cells: several tiles, ragged far edges
    want = torch.from_numpy(R.quantise(v))
    src = torch.from_numpy(img).cuda()
    n, guard = want.numel(), 259
    outs = []
    for sentinel in (0xA5, 0x5A):
        buf = torch.full((guard + n + guard,), sentinel, dtype=torch.uint8, device="cuda")
        dst = buf[guard:guard + n]
        _lib.check(lib.m2t_imresize_u8(_lib.ptr(src), img.shape[0], img.shape[1], 3, _lib.ptr(dst), s, int(up), _lib.stream_ptr()), name)
        host = buf.cpu()
        assert bool((host[:guard] == sentinel).all()) and bool((host[guard + n:] == sentinel).all())
        outs.append(host[guard:guard + n].reshape(want.shape))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], want)
    # float32: the same on planes, with a NaN pattern as the sentinel
    x = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).float().div(255.0).cuda()
    oh, ow = want.shape[0], want.shape[1]
    runs = []
    for _ in range(2):
        buf = torch.full((64 + 3 * oh * ow + 64,), float("nan"), dtype=torch.float32, device="cuda")
        dst = buf[64:64 + 3 * oh * ow]
        _lib.check(lib.m2t_imresize_f32(_lib.ptr(x), 3, img.shape[0], img.shape[1], _lib.ptr(dst), s, int(up), 0.0, _lib.stream_ptr()), name)
        host = buf.cpu()
        assert bool(host[:64].isnan().all()) and bool(host[-64:].isnan().all()) and not bool(host[64:-64].isnan().any())
        runs.append(host[64:-64])
    assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------------------- float32
def _f32_close(dev: torch.Tensor, ref64: np.ndarray):
    d = dev.double().cpu().numpy()
    return np.abs(d - ref64) <= 2.0 ** -23 * np.abs(ref64) + 1e-30


@pytest.mark.parametrize("s,up", CASES, ids=IDS)
def test_imresize_f32_is_the_fp64_reference_rounded_once(s, up):
    from m2trans_amd.resize import imresize
    g = torch.Generator().manual_seed(33 + s)
    for name, img, _ in R.u8_cases(s, up):
        if not name.startswith("rng"):
            continue
        H, W = img.shape[:2]
        planes3 = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).float().div(255.0)[None]      # [1,3,H,W]
        planes5 = torch.randn(1, 5, H, W, generator=g)
        for x in (planes3, planes5):
            ref = R.imresize(x.numpy(), s, up, axes=(2, 3))
            got = imresize(x.cuda(), s, up=up)
            assert tuple(got.shape) == ref.shape and got.dtype == torch.float32
            ok = _f32_close(got, ref)
            assert ok.all(), (name, x.shape[1], int((~ok).sum()), float(np.abs(got.double().cpu().numpy() - ref).max()))
            # clamp_max = 1: nothing outside [0, 1]; values inside are unchanged
            cl = imresize(x.cuda(), s, up=up, clamp_max=1.0)
            assert float(cl.min()) >= 0.0 and float(cl.max()) <= 1.0
            inside = (got >= 0.0) & (got <= 1.0)
            assert torch.equal(cl[inside], got[inside])
            assert torch.equal(cl[~inside], got[~inside].clamp(0.0, 1.0))
    # a batch: [N,C,H,W] is N * C planes
    x = torch.randn(2, 3, 5 * s, 7 * s, generator=g)
    assert _f32_close(imresize(x.cuda(), s, up=up), R.imresize(x.numpy(), s, up, axes=(2, 3))).all()


# ------------------------------------------------------------------------------------------------------------- error paths
def test_every_argument_error_is_raised_before_any_launch():
    _lib, lib = _lib_()
    st = _lib.stream_ptr()
    src = torch.zeros(12 * 12 * 3, dtype=torch.uint8, device="cuda")
    dst = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    fsrc = torch.zeros(12 * 12 * 3, dtype=torch.float32, device="cuda")
    fdst = torch.full((4096,), 7.0, dtype=torch.float32, device="cuda")
    s8, d8, sf, df = _lib.ptr(src), _lib.ptr(dst), _lib.ptr(fsrc), _lib.ptr(fdst)
    u8_calls = {
        "null src": (None, 12, 12, 3, d8, 2, 0), "null dst": (s8, 12, 12, 3, None, 2, 0),
        "channels 1": (s8, 12, 12, 1, d8, 2, 0), "channels 4": (s8, 12, 12, 4, d8, 2, 0),
        "scale 1": (s8, 12, 12, 3, d8, 1, 0), "scale 5": (s8, 12, 12, 3, d8, 5, 1), "scale 0": (s8, 12, 12, 3, d8, 0, 0),
        "H 0": (s8, 0, 12, 3, d8, 2, 0), "W 0": (s8, 12, 0, 3, d8, 2, 1), "H -3": (s8, -3, 12, 3, d8, 3, 0),
        "H not a multiple": (s8, 11, 12, 3, d8, 2, 0), "W not a multiple": (s8, 12, 10, 3, d8, 4, 0),
        "output height above 16384 (up)": (s8, 8193, 1, 3, d8, 2, 1), "output width above 16384 (up)": (s8, 1, 4097, 3, d8, 4, 1),
        "output width above 16384 (down)": (s8, 3, 16385 * 3, 3, d8, 3, 0),
    }
    for what, a in u8_calls.items():
        assert lib.m2t_imresize_u8(*a, st) == ARG, what
        with pytest.raises(_lib.M2TError):
            _lib.check(lib.m2t_imresize_u8(*a, st), what)
    f32_calls = {
        "null src": (None, 3, 12, 12, df, 2, 0, 0.0), "null dst": (sf, 3, 12, 12, None, 2, 0, 0.0),
        "planes 0": (sf, 0, 12, 12, df, 2, 0, 0.0), "planes 65536": (sf, 65536, 12, 12, df, 2, 0, 0.0),
        "scale 5": (sf, 3, 12, 12, df, 5, 0, 0.0), "H 0": (sf, 3, 0, 12, df, 2, 1, 0.0),
        "W not a multiple": (sf, 3, 12, 11, df, 3, 0, 0.0), "output above 16384": (sf, 1, 1, 8193, df, 2, 1, 0.0),
        "clamp_max inf": (sf, 3, 12, 12, df, 2, 0, float("inf")), "clamp_max nan": (sf, 3, 12, 12, df, 2, 1, float("nan")),
    }
    for what, a in f32_calls.items():
        assert lib.m2t_imresize_f32(*a, st) == ARG, what
        with pytest.raises(_lib.M2TError):
            _lib.check(lib.m2t_imresize_f32(*a, st), what)
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all()) and bool((fdst == 7.0).all())
    # the wrappers raise the same way
    from m2trans_amd.resize import imresize, imresize_u8
    with pytest.raises(_lib.M2TError):
        imresize_u8(src.view(12, 12, 3), 5)
    with pytest.raises(_lib.M2TError):
        imresize_u8(src.view(12, 12, 3)[:11].contiguous(), 2)
    with pytest.raises(_lib.M2TError):
        imresize(fsrc.view(1, 3, 12, 12), 2, clamp_max=float("inf"))
    with pytest.raises(_lib.M2TError):
        imresize_u8(src.view(12, 12, 3).cpu(), 2)


# ------------------------------------------------------------------------------------------------------------- datasets
@pytest.mark.parametrize("scale,patch", [(4, 48), (2, 32), (3, 48)])
def test_us1k_synthesises_its_lr_half_from_hr_alone(scale, patch):
    from m2trans_amd.datas import US1K
    imgs = R.dataset_images(scale)
    _off_ties(scale, [v for _, _, v, _ in imgs])
    assert sum(1 for hr, crop, _, _ in imgs if hr.shape != crop.shape) == 2 and len({hr.shape for hr, _, _, _ in imgs}) == 5
    synth = US1K(scale=scale, patch_size=patch, repeat=3, images=[(hr, None) for hr, _, _, _ in imgs])
    given = US1K(scale=scale, patch_size=patch, repeat=3, images=[(crop, lr) for _, crop, _, lr in imgs])
    assert torch.equal(synth.lr_pool.cpu(), torch.from_numpy(np.concatenate([lr.reshape(-1) for _, _, _, lr in imgs])))
    assert torch.equal(synth.hr_pool, given.hr_pool) and synth._geo == given._geo and len(synth) == len(given) == 15
    idx = list(range(40))
    a_lr, a_hr = synth.batch(idx, rng=random.Random(7))
    b_lr, b_hr = given.batch(idx, rng=random.Random(7))
    assert torch.equal(a_lr, b_lr) and torch.equal(a_hr, b_hr)
    # a mixed list: given LR arrays and synthesised ones side by side
    mixed = US1K(scale=scale, patch_size=patch, repeat=3,
                 images=[(crop, lr) if i % 2 else (hr, None) for i, (hr, crop, _, lr) in enumerate(imgs)])
    assert torch.equal(mixed.lr_pool, given.lr_pool) and torch.equal(mixed.hr_pool, given.hr_pool)


@pytest.mark.parametrize("scale", R.SCALES)
def test_benchmark_synthesises_its_lr_half_from_hr_alone(scale):
    from m2trans_amd.datas import Benchmark
    imgs = R.dataset_images(scale)[:3]
    _off_ties(scale, [v for _, _, v, _ in imgs])
    synth = Benchmark(scale=scale, images=[(hr, None, f"{i}.png") for i, (hr, _, _, _) in enumerate(imgs)])
    given = Benchmark(scale=scale, images=[(hr, lr, f"{i}.png") for i, (hr, _, _, lr) in enumerate(imgs)])
    assert len(synth) == len(given) == 3
    for a, b in zip(synth, given):
        assert a[2] == b[2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("scale", R.SCALES)
def test_bicubic_up_is_the_baseline_row_of_evaluate(scale):
    """evaluate(BicubicUp(s), pairs, s) is what evaluate returns for a stub serving the reference's upsampled, clamped tensors, and
    it scores strictly below the PSNR-Y of HR itself (whose squared error is 0: an infinite PSNR)."""
    from m2trans_amd.datas import Benchmark
    from m2trans_amd.metrics import evaluate, y_metrics_device
    from m2trans_amd.resize import BicubicUp
    ds = Benchmark(scale=scale, images=[(hr, None, f"{i}.png") for i, (hr, _, _, _) in enumerate(R.dataset_images(scale)[:3])])
    pairs = [(lr, hr) for lr, hr, _ in ds]
    served = iter([torch.from_numpy(np.clip(R.imresize(lr.cpu().numpy(), scale, True, axes=(2, 3)), 0.0, 1.0)).float().cuda()
                   for lr, _ in pairs])
    got = evaluate(BicubicUp(scale), pairs, scale)
    want = evaluate(lambda lr: next(served), pairs, scale)
    assert got == want, (got, want)
    assert np.isfinite(got[0]) and 10.0 < got[0] < 100.0 and 0.0 < got[1] <= 1.0
    for _, hr in pairs:
        mse_hr = float(y_metrics_device(hr, hr, scale)[0, 0])
        assert mse_hr == 0.0                                     # PSNR-Y of HR itself is +inf: the finite baseline is strictly below
    sr = BicubicUp(scale)(pairs[0][0])
    assert float(sr.min()) >= 0.0 and float(sr.max()) <= 1.0 and sr.shape == pairs[0][1].shape
    with pytest.raises(ValueError):
        BicubicUp(5)


def test_make_lr_writes_the_reference_layout(tmp_path):
    """tools/make_lr.py as a fresh child process on an HR folder with the reference's 1 000 file names (two small images and 998
    patch-sized ones): the PNG and the npy read back equal the quantised reference; a Benchmark and a US1K pointed at the written
    folders equal the ones that synthesise their LR half from the HR folder alone, with and without a cache folder."""
    from PIL import Image
    from m2trans_amd import datas
    scale, patch = 4, 48
    big = [R.dataset_images(scale)[i] for i in (0, 2)]                     # multiples of the scale: HR is stored as it is either way
    rng = np.random.default_rng(33 + scale)
    small = [rng.integers(0, 256, size=(patch, patch, 3), dtype=np.uint8) for _ in range(7)]
    hr_dir, out, cache = tmp_path / "US1K_23_HR", tmp_path / "lr", tmp_path / "cache"
    hr_dir.mkdir()
    names = [str(i).zfill(4) for i in range(1, 1001)]
    hrs = [big[k][0] if k < 2 else np.roll(small[k % 7], k, axis=1) for k in range(1000)]
    for name, hr in zip(names, hrs):
        Image.fromarray(hr, "RGB").save(hr_dir / f"{name}.png", compress_level=1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_lr.py"), "--hr", str(hr_dir), "--out", str(out), "--scale", str(scale),
                        "--npy-cache", str(cache)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["images"] == 1000 and line["scale"] == scale
    for k in (0, 1, 2, 999):
        lr = big[k][3] if k < 2 else R.quantise(R.imresize(hrs[k], scale, False))
        png = np.asarray(Image.open(out / f"X{scale}" / f"{names[k]}x{scale}.png").convert("RGB"))
        npy = np.load(cache / f"us1k_lr_x{scale}" / "rgb" / f"{names[k]}x{scale}.npy")
        assert np.array_equal(png, lr) and np.array_equal(npy, lr) and npy.dtype == np.uint8
    from_folder = datas.Benchmark(str(hr_dir), str(out), scale=scale)
    synth = datas.Benchmark(str(hr_dir), None, scale=scale)
    assert len(from_folder) == len(synth) == 1000 and sorted(from_folder.img_name) == sorted(synth.img_name) == [n + ".png" for n in names]
    where = {n: i for i, n in enumerate(synth.img_name)}
    for n in ("0001.png", "0002.png", "0003.png", "0500.png", "1000.png"):
        a, b = from_folder[from_folder.img_name.index(n)], synth[where[n]]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the HR npy cache of the folder path: present for two of the images, the PNG is read for the rest
    os.makedirs(cache / "us1k_hr" / "rgb")
    for k in (0, 2):
        np.save(cache / "us1k_hr" / "rgb" / f"{names[k]}.npy", hrs[k])
    kw = dict(scale=scale, patch_size=patch, repeat=1)
    from_files = datas.US1K(str(hr_dir), str(out), str(cache), **kw)
    idx = list(range(0, 1000, 37)) + [1, 999]
    want = from_files.batch(idx, rng=random.Random(7))
    assert len(from_files) == 1000
    for ds in (datas.US1K(str(hr_dir), None, str(cache), **kw), datas.US1K(str(hr_dir), None, None, **kw)):
        assert len(ds) == 1000 and ds._geo == from_files._geo
        assert torch.equal(ds.lr_pool, from_files.lr_pool) and torch.equal(ds.hr_pool, from_files.hr_pool)
        got = ds.batch(idx, rng=random.Random(7))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
