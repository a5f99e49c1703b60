"""GPU tests of the LR synthesis beyond bicubic (include/m2t_degrade.h, k_degrade.hip, m2trans_amd/degrade.py): every output of
m2t_degrade_patches and m2t_degrade_image_u8 against the NumPy fp64 restatement (tests/degrade_ref.py) on every bit -- no tolerance
anywhere -- the identities, determinism, the argument errors, the datasets and the resumed run."""
import copy
import ctypes as C
import itertools
import os
import random

import numpy as np
import pytest
import torch

from tests import degrade_ref as R

pytestmark = pytest.mark.gpu

SEED = (5 << 32) + 33
LEVELS = [(0.0, 0.0), (6.0, 0.0), (0.0, 0.2), (6.0, 0.2)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _call_patches(hr_images, kernels, s, lp, items, gray, seed=SEED, K=None, M=None, prefill=None, desc_edit=None, patch_size=None,
                  channels=3):
    """m2t_degrade_patches on a pool of `hr_images`; items as tests/degrade_ref.patches takes them -> (rc, lr, hr) on the host."""
    from m2trans_amd import _lib
    lib = _lib.load()
    offs = np.cumsum([0] + [im.size for im in hr_images])
    pool = torch.from_numpy(np.concatenate([im.reshape(-1) for im in hr_images])).cuda()
    bank = torch.from_numpy(np.ascontiguousarray(kernels, dtype=np.float64)).cuda()
    n = len(items)
    desc = np.zeros((n, _lib.DEGRADE_DESC_COLS), dtype=np.int64)
    lev = np.zeros((n, 2))
    for k, (img, lx, ly, flags, index, sa, ss, nid) in enumerate(items):
        H, W, _ = hr_images[img].shape
        desc[k, :8] = (offs[img], H, W, lx, ly, flags, index, nid - (1 << 64) if nid >= 1 << 63 else nid)
        lev[k] = (sa, ss)
        desc[k, 10] = int(gray)
    desc[:, 8:10] = lev.view(np.int64)
    if desc_edit is not None:
        desc_edit(desc)
    fill = float("nan") if prefill is None else prefill
    lr = torch.full((n, 3, lp, lp), fill, dtype=torch.float32, device="cuda")
    hr = torch.full((n, 3, lp * s, lp * s), fill, dtype=torch.float32, device="cuda")
    rc = lib.m2t_degrade_patches(_lib.ptr(pool), _lib.ptr(bank), kernels.shape[0] if M is None else M, kernels.shape[1] if K is None else K,
                                 desc.ctypes.data_as(C.c_void_p), n, channels, lp * s if patch_size is None else patch_size, s, seed,
                                 _lib.ptr(lr), _lib.ptr(hr), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, lr.cpu().numpy(), hr.cpu().numpy()


def _image(H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- patches
@pytest.mark.parametrize("s,K", [(2, 2), (2, 20), (3, 1), (3, 21), (4, 2), (4, 20)])
def test_patches_equal_the_restatement_on_every_bit(s, K):
    """HR 36 x 40 (36 x 39 at x3), lp = 8, the corner (0, 0) and the largest admissible one (reflection on all four sides with the
    largest K), all 8 flag values, the four level pairs, 33 items per call (two by-value chunks), gray noise on and off."""
    H, W, lp = 36, 39 if s == 3 else 40, 8
    images = [_image(H, W, 10 * s + k) for k in range(2)]
    kernels = R.bank(s, M=3, K=K, seed=11)[0]
    far = (W // s - lp, H // s - lp)
    combos = list(itertools.product(((0, 0), far), range(8), LEVELS))            # 64
    random.Random(s * K).shuffle(combos)
    combos += combos[:2]
    items = [(k % 2, c[0], c[1], f, k % 3, sa, ss, (k * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) for k, (c, f, (sa, ss)) in enumerate(combos)]
    assert len(items) == 66
    for gray, part in ((True, items[:33]), (False, items[33:])):
        rc, lr, hr = _call_patches(images, kernels, s, lp, part, gray)
        assert rc == 0
        want_lr, want_hr = R.patches(images, kernels, s, lp, part, gray, SEED)
        bad = np.argwhere(_bits(lr) != _bits(want_lr))
        assert bad.size == 0, (len(bad), bad[:4].tolist(), part[bad[0][0]])
        assert np.array_equal(_bits(hr), _bits(want_hr))


@pytest.mark.parametrize("s", [2, 4])
def test_multi_fold_an_image_narrower_than_the_kernel(s):
    images = [_image(8, 12, s)]
    kernels = R.bank(s, M=2, K=20, seed=3)[0]
    far = (12 // s - 2, 8 // s - 2)
    items = [(0, c[0], c[1], f, f % 2, 5.0, 0.1, 77 + f) for c in ((0, 0), far) for f in range(8)]
    rc, lr, hr = _call_patches(images, kernels, s, 2, items, True)
    want_lr, want_hr = R.patches(images, kernels, s, 2, items, True, SEED)
    assert rc == 0 and np.array_equal(_bits(lr), _bits(want_lr)) and np.array_equal(_bits(hr), _bits(want_hr))


# ------------------------------------------------------------------------------------------------------------- whole image
@pytest.mark.parametrize("s,lh,lw,extra", [(2, 13, 19, (1, 0)), (3, 33, 17, (2, 1)), (4, 33, 17, (0, 3)), (3, 13, 19, (0, 0))],
                         ids=["x2-13x19", "x3-33x17", "x4-33x17", "x3-13x19"])
def test_whole_image_equals_the_restatement_on_every_byte(s, lh, lw, extra):
    from m2trans_amd.degrade import Degradation
    hr = _image(lh * s + extra[0], lw * s + extra[1], lh + s)
    D = Degradation(s, bank=4, seed=SEED, gray_noise=True)
    E = Degradation(s, bank=4, seed=SEED, gray_noise=False)
    dev = torch.from_numpy(hr).cuda()
    for obj, gray in ((D, True), (E, False)):
        for index, sa, ss, nid in ((0, 0.0, 0.0, 0), (3, 4.0, 0.15, (1 << 63) + 9), (2, 7.0, 0.0, 5)):
            got = obj.apply_image(dev, index=index, sigma_add=sa, sigma_speckle=ss, noise_id=nid).cpu().numpy()
            want = R.image_u8(hr, obj.kernels[index], s, sa, ss, gray, nid, SEED)
            assert got.shape == (lh, lw, 3) and np.array_equal(got, want), (gray, index, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------------------- identities
def test_delta_kernel_without_noise_is_crop_patches_of_the_decimated_image():
    from m2trans_amd.datas import US1K
    from m2trans_amd.degrade import Degradation
    hr = _image(36, 39, 1)
    delta = np.zeros((1, 3, 3))
    delta[0, 1, 1] = 1.0
    D = Degradation(3, kernels=delta, noise=(0, 0), speckle=(0, 0))
    plain = US1K(images=[(hr, np.ascontiguousarray(hr[1::3, 1::3]))], scale=3, patch_size=24, repeat=1, device="cuda")
    deg = US1K(images=[(hr, None)], scale=3, patch_size=24, repeat=1, device="cuda", degradation=D)
    assert deg.lr_pool is None
    draws = [((f * 5) % 6, (f * 3) % 5, f) for f in range(8)]       # corners 0 .. 5 and 0 .. 4, the largest ones included
    lr_a, hr_a = plain.batch([0] * 8, draws=draws)
    lr_b, hr_b = deg.batch([0] * 8, draws=draws)
    assert torch.equal(lr_a.view(torch.int32), lr_b.view(torch.int32)) and torch.equal(hr_a.view(torch.int32), hr_b.view(torch.int32))


def test_constant_images_and_the_clamp():
    kernels = R.bank(4, M=2, K=20, seed=2)[0]
    for value in (0, 77, 255):
        img = np.full((40, 48, 3), value, dtype=np.uint8)
        items = [(0, 1, 0, f, f % 2, 0.0, 0.0, f) for f in range(8)]
        rc, lr, _ = _call_patches([img], kernels, 4, 8, items, True)
        assert rc == 0 and np.array_equal(_bits(lr), _bits(np.full_like(lr, np.float32(value) / np.float32(255.0))))
    for value in (0, 255):
        img = np.full((40, 48, 3), value, dtype=np.uint8)
        items = [(0, 1, 0, f, f % 2, 20.0, 0.0, f) for f in range(8)]
        rc, lr, _ = _call_patches([img], kernels, 4, 8, items, False)
        assert rc == 0 and float(lr.min()) >= 0.0 and float(lr.max()) <= 1.0
        assert len(np.unique(lr)) > 5                            # half of the variates are cut off, the others are there


# ------------------------------------------------------------------------------------------------------------- determinism
def test_determinism_noise_id_and_full_overwrite():
    images = [_image(36, 40, 4)]
    kernels = R.bank(2, M=2, K=8, seed=2)[0]
    items = [(0, k % 5, k % 3, k % 8, k % 2, 5.0, 0.1, 100 + k) for k in range(33)]
    rc, lr1, hr1 = _call_patches(images, kernels, 2, 8, items, True)
    rc2, lr2, hr2 = _call_patches(images, kernels, 2, 8, items, True, prefill=-3.0)
    assert rc == rc2 == 0 and np.array_equal(_bits(lr1), _bits(lr2)) and np.array_equal(_bits(hr1), _bits(hr2))
    assert np.isfinite(lr1).all() and np.isfinite(hr1).all()                       # the NaN prefill is gone
    other = [it[:7] + (it[7] + (1 << 32),) for it in items]
    _, lr3, hr3 = _call_patches(images, kernels, 2, 8, other, True)
    assert np.array_equal(_bits(hr1), _bits(hr3))
    assert all(not np.array_equal(lr1[k], lr3[k]) for k in range(33))
    _, lr4, _ = _call_patches(images, kernels, 2, 8, items, True, seed=SEED + 1)
    assert not np.array_equal(lr1, lr4)


# ------------------------------------------------------------------------------------------------------------- argument errors
def _set(col, value, row=1):
    def edit(desc):
        desc[row, col] = value
    return edit


def _level(col, value):
    def edit(desc):
        desc[1, col] = np.array([value]).view(np.int64)[0]
    return edit


def test_argument_errors_come_before_any_launch():
    from m2trans_amd import _lib
    from m2trans_amd._lib import M2TError
    from m2trans_amd.degrade import Degradation
    lib = _lib.load()
    images = [_image(36, 40, 4)]
    k2, k3 = R.bank(2, M=2, K=8, seed=2)[0], R.bank(3, M=2, K=7, seed=2)[0]
    items = [(0, 1, 2, 3, 1, 5.0, 0.1, 9)] * 3

    def refused(what, s=2, kernels=k2, **kw):
        rc, lr, hr = _call_patches(images, kernels, s, 8 if s == 2 else 4, items, True, **kw)
        assert rc == -2, (what, rc)
        assert np.isnan(lr).all() and np.isnan(hr).all(), what                    # nothing was launched
        return lib.m2t_last_error_string().decode()

    assert "scale" in refused("scale 5", s=5)
    assert "scale" in refused("scale 1", s=1)
    assert "parity" in refused("odd K at x2", K=7)
    assert "parity" in refused("even K at x3", s=3, kernels=k3, K=8)
    assert "parity" in refused("K 22", K=22)
    assert "parity" in refused("K 0", K=0)
    assert "empty" in refused("M 0", M=0)
    assert "bank index" in refused("bank index M", desc_edit=_set(6, 2))
    assert "bank index" in refused("bank index -1", desc_edit=_set(6, -1))
    assert "outside the image" in refused("lx beyond", desc_edit=_set(3, 13))
    assert "outside the image" in refused("ly beyond", desc_edit=_set(4, 11))
    assert "out of range" in refused("lx < 0", desc_edit=_set(3, -1))
    assert "out of range" in refused("offset < 0", desc_edit=_set(0, -1))
    assert "flags" in refused("flags 8", desc_edit=_set(5, 8))
    assert "flags" in refused("flags 8, last item", desc_edit=_set(5, 8, row=2))
    for col in (8, 9):
        for v in (-1.0, float("nan"), float("inf")):
            assert "level" in refused(f"level {v}", desc_edit=_level(col, v))
    assert "gray" in refused("gray 2", desc_edit=_set(10, 2))
    assert "multiple" in refused("patch 15", patch_size=15)
    assert "3 channels" in refused("one channel", channels=1)
    # the whole-image entry, through the Python method
    D = Degradation(2, kernels=k2, seed=3)
    dev = torch.from_numpy(images[0]).cuda()
    out = torch.full((18, 20, 3), 171, dtype=torch.uint8, device="cuda")
    for kw in (dict(index=2), dict(index=-1), dict(sigma_add=-1.0), dict(sigma_speckle=float("nan")), dict(sigma_add=float("inf"))):
        with pytest.raises(M2TError, match="m2t_degrade_image_u8"):
            D.apply_image(dev, out=out, **kw)
    torch.cuda.synchronize()
    assert bool((out == 171).all())
    with pytest.raises(M2TError, match="smaller"):
        D.apply_image(dev[:1])
    with pytest.raises(M2TError, match="uint8"):
        D.apply_image(dev.float())
    one = C.c_void_p(8)
    assert lib.m2t_degrade_image_u8(one, 1, 40, 3, one, 2, 8, 0, 2, 0, 0, 0.0, 0.0, 1, one, None) == -2
    assert lib.m2t_degrade_image_u8(one, 36, 40, 3, one, 2, 7, 0, 2, 0, 0, 0.0, 0.0, 1, one, None) == -2
    assert lib.m2t_degrade_image_u8(one, 36, 40, 3, one, 2, 8, 0, 2, 0, 0, 0.0, 0.0, 2, one, None) == -2
    assert lib.m2t_degrade_image_u8(None, 36, 40, 3, one, 2, 8, 0, 2, 0, 0, 0.0, 0.0, 1, one, None) == -2


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


def test_us1k_batch_equals_the_restatement_driven_by_a_copy():
    from m2trans_amd.datas import US1K
    from m2trans_amd.degrade import Degradation
    imgs = _train_images()
    D = Degradation(4, bank=8, ksize=10, noise=(1.0, 9.0), speckle=(0.0, 0.2), seed=SEED)
    twin = copy.deepcopy(D)
    ds = US1K(images=[(im, None) for im in imgs], scale=4, patch_size=32, repeat=2, device="cuda", degradation=D)
    plain = US1K(images=[(im, None) for im in imgs], scale=4, patch_size=32, repeat=2, device="cuda")
    assert ds.lr_pool is None and len(ds) == 6
    idx = [4, 0, 5, 2, 1]
    random.seed(7)
    lr, hr = ds.batch(idx)
    after = random.getstate()
    random.seed(7)
    items = []
    for i in idx:
        lx, ly, flags = plain.draw(i)
        items.append((i % 3, lx, ly, flags) + twin.draw())
    assert random.getstate() == after                             # the degradation draws nothing from the global generator
    want_lr, want_hr = R.patches(imgs, twin.kernels, 4, 8, items, True, SEED)
    assert np.array_equal(_bits(lr.cpu().numpy()), _bits(want_lr)) and np.array_equal(_bits(hr.cpu().numpy()), _bits(want_hr))
    # the HR batches of a degraded and a plain dataset under the same seed
    random.seed(7)
    lr_p, hr_p = plain.batch(idx)
    assert torch.equal(hr_p.view(torch.int32), hr.view(torch.int32)) and not torch.equal(lr_p, lr)
    assert D.draw()[3] == 5 == twin.draw()[3]


def test_benchmark_is_the_same_at_every_construction_and_pairs_are_refused():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.datas import US1K, Benchmark
    from m2trans_amd.degrade import BENCHMARK_NOISE_ID, Degradation
    imgs = _train_images()
    D = Degradation(4, bank=8, ksize=10, noise=(1.0, 9.0), speckle=(0.0, 0.2), seed=SEED)
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
        want = R.image_u8(hr, D.kernels[index], 4, sa, ss, True, BENCHMARK_NOISE_ID + k, SEED)
        assert np.array_equal(_bits(la[0].cpu().numpy()), _bits(R.to_tensor(want)))
    small = np.ascontiguousarray(imgs[0][::4, ::4])
    with pytest.raises(M2TError, match="HR-only"):
        US1K(images=[(imgs[0], small)], scale=4, patch_size=32, device="cuda", degradation=D)
    with pytest.raises(M2TError, match="HR-only"):
        Benchmark(images=[(imgs[0], small, "a.png")], scale=4, device="cuda", degradation=D)
    with pytest.raises(M2TError, match="HR-only"):
        US1K("hr", "lr", "cache", scale=4, patch_size=32, device="cuda", degradation=D)
    with pytest.raises(M2TError, match="x4"):
        US1K(images=[(imgs[0], None)], scale=2, patch_size=32, device="cuda", degradation=D)


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
    D = Degradation(2, bank=8, noise=(1.0, 9.0), speckle=(0.0, 0.2), seed=SEED)
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


def test_resume_with_degradation_repeats_the_uninterrupted_run(tmp_path):
    full = _fit(tmp_path / "full")
    assert full["steps"] == 6 and full["D"].get_state()["noise_id"] == 12
    ckpt = torch.load(tmp_path / "full" / "models" / "model_x2_1.pt", map_location="cpu", weights_only=False)
    assert set(ckpt["m2t_rng"]) == {"random", "numpy", "torch", "loader", "degradation"} and ckpt["m2t_rng"]["degradation"]["noise_id"] == 6
    first = _fit(tmp_path / "cut", last_epoch=1)
    assert first["steps"] == 3 and os.listdir(tmp_path / "cut" / "models") == ["model_x2_1.pt"]
    second = _fit(tmp_path / "cut", resume=str(tmp_path / "cut"))                   # fresh objects: the state comes from the file
    assert any("resume training from epoch 2" in l for l in second["lines"])
    assert second["steps"] == 6 and second["D"].get_state() == full["D"].get_state()
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(second[k], full[k]), k
    assert second["stat"] == full["stat"]
    assert not torch.equal(first["params"], full["params"])


# ------------------------------------------------------------------------------------------------------------- the tool
def test_make_lr_writes_the_degraded_folder(tmp_path, capsys):
    """tools/make_lr.py --degradation (its main(), in this process): the PNGs equal the restatement in sorted file order, which is
    what a Benchmark with the same Degradation computes."""
    import importlib.util
    import json
    import yaml
    from PIL import Image
    from m2trans_amd.degrade import BENCHMARK_NOISE_ID, Degradation
    imgs = _train_images()[:2]
    hr_dir = tmp_path / "hr"
    hr_dir.mkdir()
    Image.fromarray(imgs[0][:50, :67].copy(), "RGB").save(hr_dir / "b.png")
    Image.fromarray(imgs[1], "RGB").save(hr_dir / "a.png")
    cfg = {"bank": 8, "ksize": 7, "noise": [1.0, 9.0], "speckle": [0.0, 0.2], "seed": 12}
    (tmp_path / "deg.yml").write_text(yaml.safe_dump({"degradation": cfg}))
    spec = importlib.util.spec_from_file_location("make_lr_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 "tools", "make_lr.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(["--hr", str(hr_dir), "--out", str(tmp_path / "lr"), "--scale", "3", "--degradation", str(tmp_path / "deg.yml")])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["images"] == 2 and line["degradation"] is True
    D = Degradation(3, bank=8, ksize=7, noise=(1.0, 9.0), speckle=(0.0, 0.2), seed=12)
    rng = random.Random(12)
    for k, (name, hr) in enumerate((("a", imgs[1]), ("b", imgs[0][:50, :67]))):
        hr = hr[:hr.shape[0] // 3 * 3, :hr.shape[1] // 3 * 3]
        index, sa, ss = D.draw_levels(rng)
        want = R.image_u8(hr, D.kernels[index], 3, sa, ss, True, BENCHMARK_NOISE_ID + k, 12)
        got = np.asarray(Image.open(tmp_path / "lr" / "X3" / f"{name}x3.png").convert("RGB"))
        assert np.array_equal(got, want), name


def test_the_config_key_reaches_the_training_set_and_the_eval_folders(tmp_path):
    """train.resolve_config + build_datasets from two folders: one Degradation, built from the mapping, behind both datasets."""
    from PIL import Image
    from m2trans_amd import train as T
    imgs = _train_images()
    (tmp_path / "hr").mkdir()
    (tmp_path / "val").mkdir()
    for k, im in enumerate(imgs):
        Image.fromarray(im, "RGB").save(tmp_path / "hr" / f"{k}.png")
    Image.fromarray(imgs[0][:64, :64].copy(), "RGB").save(tmp_path / "val" / "v.png")
    cfg = {"scale": 2, "patch_size": 64, "batch_size": 2, "epochs": 1, "lr": 1e-4, "eta_min": 1e-6, "log_every": 1, "test_every": 1,
           "training_dataset": "folder", "train_hr_path": str(tmp_path / "hr"), "eval_folders": {"mine": str(tmp_path / "val")},
           "degradation": {"bank": 4, "ksize": 6, "noise": [2.0, 2.0], "speckle": [0.0, 0.0], "seed": 21}}
    train, valid = T.build_datasets(T.resolve_config(cfg)["data"])
    D = train.degradation
    assert D is not None and valid[0][1].degradation is D and (len(D), D.ksize, D.noise, D.seed) == (4, 6, (2.0, 2.0), 21)
    assert train.lr_pool is None
    random.seed(3)
    lr, hr = train.batch([0, 1])
    from m2trans_amd.degrade import from_config
    twin = from_config(2, cfg["degradation"])                  # a second object from the same mapping: the same bank and draws
    random.seed(3)
    items = []
    for i in (0, 1):
        lx, ly, flags = train.draw(i)
        items.append((i, lx, ly, flags) + twin.draw())
    want_lr, want_hr = R.patches(imgs, twin.kernels, 2, 32, items, True, 21)
    assert np.array_equal(_bits(lr.cpu().numpy()), _bits(want_lr)) and np.array_equal(_bits(hr.cpu().numpy()), _bits(want_hr))
    v_lr, v_hr, name = valid[0][1][0]
    assert name == "v.png" and tuple(v_lr.shape) == (1, 3, 32, 32) and tuple(v_hr.shape) == (1, 3, 64, 64)
