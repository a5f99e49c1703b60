"""GPU tests of the training entry (include/m2t_train.h, k_train.hip, m2trans_amd/train.py): the step meter and the preview strip
against the restatements of tests/train_ref.py, bit for bit, and the epoch loop `fit` against a hand-written loop around
`TrainStep.step`: the loop adds nothing to the arithmetic, resumes exactly, logs the sequential fp64 means and reads no device
value inside its batch loop.  Every comparison here is an equality of bits: there is no tolerance to choose."""
import glob
import math
import os
import random

import numpy as np
import pytest
import torch

from tests import train_ref as R

pytestmark = pytest.mark.gpu

SCALE, PATCH, BATCH, REPEAT, EPOCHS, LR0, ETA_MIN, SEED = 4, 128, 2, 2, 2, 1e-4, 1e-6, 33


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------------------- the meter
def _meter_columns(n: int, device):
    rng = np.random.RandomState(7)
    c0 = (rng.rand(n) * 10.0 ** rng.randint(-6, 6, n)).astype(np.float32)              # a sum whose bits depend on the order
    c1 = rng.randn(n) * 10.0 ** rng.randint(-9, 9, n)
    c1[11] = 1e300                                                                      # rounds to +inf in the float32 ring
    c3 = rng.rand(n).astype(np.float32)
    c3[3], c3[5] = np.nan, np.inf
    c4 = np.full(n, 0.1, np.float32)
    host = [c0, c1, None, c3, c4]
    dev = [None if c is None else torch.from_numpy(c).to(device) for c in host]
    return host, dev


def _run_meter(meter, dev, n):
    for step in range(n):
        meter.update([None if c is None else c[step:step + 1] for c in dev], step)
    torch.cuda.synchronize()
    return meter.record.cpu().numpy().copy(), meter.ring.cpu().numpy().copy()


def test_meter_matches_the_sequential_fp64_restatement_bit_for_bit():
    from m2trans_amd.train import StepMeter
    n, rows = 40, 16                                                                    # the ring wraps twice
    host, dev = _meter_columns(n, "cuda")
    meter = StepMeter(["f32", "f64", "absent", "turns", "const"], "cuda", ring_rows=rows)
    rec, ring = _run_meter(meter, dev, n)
    ref = R.RefMeter(5, rows)
    for step in range(n):
        ref.update([None if c is None else c[step] for c in host], step)
    assert np.array_equal(_bits(rec), _bits(ref.record)), (rec, ref.record)
    assert np.array_equal(np.isnan(ring), np.isnan(ref.ring))
    keep = ~np.isnan(ring)
    assert np.array_equal(_bits(ring)[keep], _bits(ref.ring)[keep])
    # what the record says, in words
    assert rec[3, 1] == n - 2 and rec[3, 2] == 2 and math.isfinite(rec[3, 0]) and rec[3, 4] <= 1.0
    assert rec[2].tolist() == [0, 0, 0, math.inf, -math.inf, 0, 0, 0] and np.isnan(ring[:, 3]).all()
    assert rec[4, 0] == sum([float(np.float32(0.1))] * n) and rec[4, 3] == rec[4, 4] == rec[4, 5] == float(np.float32(0.1))
    assert sorted(ring[:, 0].tolist()) == [float(s) for s in range(n - rows, n)] and np.isinf(ring[:, 2]).sum() == 0
    # ... independent of what the buffers held before: poison, reset, run again
    meter.record.fill_(float("nan"))
    meter.ring.fill_(float("nan"))
    meter.reset()
    rec2, ring2 = _run_meter(meter, dev, n)
    assert rec2.tobytes() == rec.tobytes() and ring2.tobytes() == ring.tobytes()
    # ... and a second, identical run on fresh buffers gives identical bytes
    rec3, ring3 = _run_meter(StepMeter(["f32", "f64", "absent", "turns", "const"], "cuda", ring_rows=rows), dev, n)
    assert rec3.tobytes() == rec.tobytes() and ring3.tobytes() == ring.tobytes()
    named = meter.read()
    assert named["turns"]["nonfinite"] == 2.0 and named["f64"]["max"] == 1e300 and named["const"]["count"] == n
    curves = meter.curves()
    assert curves[:, 0].tolist() == [float(s) for s in range(n - rows, n)]


def test_meter_ring_rounds_a_large_double_to_infinity():
    from m2trans_amd.train import StepMeter
    meter = StepMeter(["v"], "cuda", ring_rows=2)
    meter.update([torch.tensor([1e300], dtype=torch.float64, device="cuda")], 0)
    assert meter.ring.cpu()[0].tolist() == [0.0, math.inf] and meter.read()["v"]["sum"] == 1e300


# ------------------------------------------------------------------------------------------------------------- the preview
@pytest.mark.parametrize("rgb_range", [1.0, 255.0])
@pytest.mark.parametrize("h,w", [(5, 7), (33, 40)])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_preview_strip_equals_the_integer_restatement_byte_for_byte(s, h, w, rgb_range):
    from m2trans_amd.train import preview_strip
    rng = np.random.RandomState(100 * s + h)
    lr = (rng.rand(3, h, w) * rgb_range).astype(np.float32)
    sr = ((rng.rand(3, h * s, w * s) * 1.2 - 0.1) * rgb_range).astype(np.float32)
    hr = (rng.rand(3, h * s, w * s) * rgb_range).astype(np.float32)
    planted = [np.nan, -0.3 * rgb_range, 1.7 * rgb_range, rgb_range, np.inf, -np.inf]
    for a in (lr, sr, hr):
        flat = a.reshape(-1)
        where = rng.choice(flat.size, size=3 * len(planted), replace=False)
        flat[where] = np.tile(np.array(planted, np.float32), 3)
    lr[:, 0, 0], lr[:, h - 1, w - 1] = np.float32(rgb_range), np.nan          # (the clamped corners)
    got = preview_strip(torch.from_numpy(lr).cuda(), torch.from_numpy(sr).cuda(), torch.from_numpy(hr).cuda(), rgb_range)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h * s, 3 * w * s, 3)
    want = R.preview_strip(lr, sr, hr, rgb_range)
    got = got.cpu().numpy()
    diff = np.argwhere(got != want)
    assert diff.size == 0, (len(diff), diff[:5].tolist(), got[tuple(diff[0])], want[tuple(diff[0])])
    assert (got[0, 0] == 255).all() and (got[h * s - 1, w * s - 1] == 0).all()


# ------------------------------------------------------------------------------------------------------------- the loop
def _images():
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:160, 0:192]
    out = []
    for k in range(3):
        base = 120 + 80 * np.sin(xx / (7.0 + k) + k) * np.cos(yy / (11.0 - k))
        img = np.stack([base, base * 0.9, base * 0.8], axis=2) + rng.randint(0, 30, size=(160, 192, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def _objects(**ts_kw):
    from m2trans_amd.datas import US1K, Benchmark
    from m2trans_amd.train_step import TrainStep
    from tests.gpu_util import build_model
    model, _ = build_model(SCALE, 1, "fp32")
    ts = TrainStep(model, lr=LR0, world_size=1, **ts_kw)
    imgs = _images()
    ds = US1K(images=[(im, None) for im in imgs], scale=SCALE, patch_size=PATCH, repeat=REPEAT, device="cuda")
    # (LR 24 x 24 and 24 x 32: the model pads to a multiple of 32 by reflection, which needs pad < size)
    valid = [("mine", Benchmark(images=[(imgs[0][:96, :96].copy(), None, "a.png"), (imgs[1][:96, :128].copy(), None, "b.png")],
                                scale=SCALE, device="cuda"))]
    assert len(ds) == 6
    return model, ts, ds, valid


def _state(model, ts):
    torch.cuda.synchronize()
    return {"params": model.flat_params.detach().cpu().clone(), "exp_avg": ts.exp_avg.cpu().clone(),
            "exp_avg_sq": ts.exp_avg_sq.cpu().clone(), "step_count": ts.step_count}


def _same_state(a, b):
    assert a["step_count"] == b["step_count"]
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


def _fit(out_dir, objects=None, **kw):
    """fit on the test's setup; returns (state, stat_dict, the on_log infos, the preview strips the kernel produced)."""
    from m2trans_amd import train as T
    model, ts, ds, valid = objects or _objects()
    infos, strips, lines = [], [], []
    real = T.preview_strip

    def recording(*a, **k):
        strips.append(real(*a, **k).cpu().numpy())
        return torch.from_numpy(strips[-1]).cuda()
    args = dict(epochs=EPOCHS, batch_size=BATCH, lr0=LR0, eta_min=ETA_MIN, log_every=1, test_every=1, out_dir=str(out_dir), cutmix=True,
                patch_size=PATCH, preview_every=2, seed=SEED, ring_rows=8, log=lines.append, on_log=infos.append)
    args.update(kw)
    T.preview_strip = recording
    try:
        stat = T.fit(model, ts, ds, valid, **args)
    finally:
        T.preview_strip = real
    return {"state": _state(model, ts), "stat": stat, "infos": infos, "strips": strips, "lines": lines, "ts": ts, "model": model}


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    """The uninterrupted run: two epochs of three batches, cutmix on, a log point per batch, validation and a checkpoint per epoch."""
    out = tmp_path_factory.mktemp("full")
    r = _fit(out)
    r["dir"] = str(out)
    return r


@pytest.fixture(scope="module")
def hand_run():
    """The same arithmetic written out by hand: the generators seeded alike, loader / cutmix / set_lr / step, nothing else.  It reads
    the loss values after every step (a second, identical run: the reading changes no arithmetic)."""
    from m2trans_amd import augment
    from m2trans_amd.train_step import cosine_lr
    model, ts, ds, _ = _objects()
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    g = torch.Generator()
    g.manual_seed(SEED)
    per_step = []
    for epoch in range(1, EPOCHS + 1):
        ts.set_lr(cosine_lr(epoch - 1, LR0, ETA_MIN, EPOCHS))
        n = 0
        for lr, hr in ds.loader(BATCH, shuffle=True, generator=g):
            lr, hr = augment.cutmix(lr, hr, 1.0, np.random.randint(1, 5), SCALE)
            ts.step(lr, hr)
            per_step.append((epoch, n, float(ts.loss), float(ts.l1_loss)))
            n += 1
        assert n == 3
    return {"state": _state(model, ts), "per_step": per_step}


def test_the_loop_adds_nothing_to_the_arithmetic(full_run, hand_run):
    _same_state(full_run["state"], hand_run["state"])
    assert full_run["state"]["step_count"] == 6
    assert float(hand_run["state"]["exp_avg"].abs().max()) > 0.0


def test_logged_means_are_the_sequential_fp64_means(full_run, hand_run):
    infos = full_run["infos"]
    assert [(i["epoch"], i["iter"]) for i in infos] == [(e, n) for e, n, _, _ in hand_run["per_step"]]
    losses = []
    for info, (epoch, n, _, _) in zip(infos, hand_run["per_step"]):
        rows = [p for p in hand_run["per_step"] if p[0] == epoch and p[1] <= n]
        s_loss = s_pix = 0.0
        for _, _, a, b in rows:                                # sequential fp64 sums, in step order
            s_loss, s_pix = s_loss + a, s_pix + b
        assert info["means"]["loss"] == s_loss / (n + 1) and info["means"]["pixel"] == s_pix / (n + 1), (epoch, n)
        assert info["means"]["clip"] == 0.0 and info["record"]["clip"]["count"] == 0.0
        assert info["record"]["loss"]["last"] == rows[-1][2] and info["record"]["loss"]["count"] == n + 1
        losses.append(s_loss / (n + 1) / (n + 1))              # the reference divides twice (train.py:244-248)
    assert full_run["stat"]["losses"] == losses
    # the printed line carries the same means, rounded
    text = [l for l in full_run["lines"] if l.startswith("Epoch:")]
    assert len(text) == 6 and text[0].startswith("Epoch:1, 2/6, loss: {:.4f}, L1loss: {:.4f}, CLIPloss: 0.00000000 time: ".format(
        infos[0]["means"]["loss"], infos[0]["means"]["pixel"]))
    # the ring of the second epoch: the global step index and the values rounded to float32
    curves = infos[-1]["meter"].curves()
    assert curves[:, 0].tolist() == [3.0, 4.0, 5.0]
    assert curves[:, 1].tolist() == [float(np.float32(p[2])) for p in hand_run["per_step"][3:]]
    assert torch.isnan(curves[:, 3]).all()


def test_files_of_a_run(full_run):
    import yaml
    from PIL import Image
    from m2trans_amd.checkpoint import import_checkpoint
    out = full_run["dir"]
    assert sorted(os.listdir(os.path.join(out, "models"))) == ["model_x4_1.pt", "model_x4_2.pt"]
    ckpt = torch.load(os.path.join(out, "models", "model_x4_1.pt"), map_location="cpu", weights_only=False)
    assert ckpt["epoch"] == 1 and set(ckpt["m2t_rng"]) == {"random", "numpy", "torch", "loader"}
    assert ckpt["scheduler_state_dict"]["last_epoch"] == 0 and ckpt["optimizer_state_dict"]["param_groups"][0]["lr"] == LR0
    model, ts, _, _ = _objects()
    assert import_checkpoint(ckpt, model, ts) == 2 and ts.step_count == 3 and ts.lr == LR0
    assert float(ts.exp_avg.abs().max()) > 0.0
    stat = yaml.safe_load(open(os.path.join(out, "stat_dict.yml")))
    assert stat == full_run["stat"] and stat["epochs"] == 2 and len(stat["mine"]["psnrs"]) == 2 and len(stat["losses"]) == 6
    assert stat["mine"]["best_psnr"]["epoch"] in (1, 2) and stat["mine"]["psnrs"][0] > 0.0
    pngs = sorted(glob.glob(os.path.join(out, "preview", "*.png")))
    assert [os.path.basename(p) for p in pngs] == ["epoch0001_iter000001.png", "epoch0002_iter000001.png"]
    assert len(full_run["strips"]) == 2
    for p, strip in zip(pngs, full_run["strips"]):
        assert strip.shape == (PATCH, 3 * PATCH, 3)
        assert np.array_equal(np.asarray(Image.open(p)), strip)                # the PNG decodes to the kernel's bytes
        assert strip[:, 2 * PATCH:].std() > 1.0                                # (the HR third is an image, not a constant)


def test_resume_repeats_the_uninterrupted_run(full_run, tmp_path):
    first = _fit(tmp_path, last_epoch=1)
    assert first["state"]["step_count"] == 3 and os.listdir(tmp_path / "models") == ["model_x4_1.pt"]
    assert first["infos"] and all(i["epoch"] == 1 for i in first["infos"])
    second = _fit(tmp_path, resume=str(tmp_path))                              # fresh objects
    assert any("resume training from epoch 2" in l for l in second["lines"])
    _same_state(second["state"], full_run["state"])
    assert second["stat"] == full_run["stat"]
    want = [i["means"] for i in full_run["infos"] if i["epoch"] == 2]
    assert [i["means"] for i in second["infos"]] == want and len(want) == 3
    assert second["ts"].scheduler_last_epoch == full_run["ts"].scheduler_last_epoch == 2
    assert sorted(os.listdir(tmp_path / "models")) == ["model_x4_1.pt", "model_x4_2.pt"]


def test_a_checkpoint_without_m2t_rng_resumes_the_reference_way(full_run, tmp_path):
    ckpt = torch.load(os.path.join(full_run["dir"], "models", "model_x4_1.pt"), map_location="cpu", weights_only=False)
    del ckpt["m2t_rng"]
    os.makedirs(tmp_path / "models")
    torch.save(ckpt, tmp_path / "models" / "model_x4_1.pt")
    r = _fit(tmp_path, resume=str(tmp_path), test_every=5)
    assert any("carries no m2t_rng entry" in l for l in r["lines"])
    assert any("Epoch: 2, lr: [0.0001]" in l for l in r["lines"])              # the saved rate, re-used (train.py:101-103)
    assert r["state"]["step_count"] == 6


def test_extra_columns_with_an_optional_term_and_the_gradient_norm(tmp_path):
    from m2trans_amd import augment
    from m2trans_amd.train_step import cosine_lr
    kw = dict(lambda_ssim=0.25, track_grad_norm=True, max_grad_norm=0.05)
    r = _fit(tmp_path, objects=_objects(**kw), epochs=1, test_every=5, preview_every=100)
    assert list(r["infos"][0]["means"]) == ["loss", "pixel", "clip", "ssim", "grad_norm", "clip_coef"]
    model, ts, ds, _ = _objects(**kw)
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    g = torch.Generator()
    g.manual_seed(SEED)
    ts.set_lr(cosine_lr(0, LR0, ETA_MIN, 1))
    sums = {n: 0.0 for n in ("loss", "pixel", "ssim", "grad_norm", "clip_coef")}
    for n, (lr, hr) in enumerate(ds.loader(BATCH, shuffle=True, generator=g)):
        lr, hr = augment.cutmix(lr, hr, 1.0, np.random.randint(1, 5), SCALE)
        ts.step(lr, hr)
        for name, t in (("loss", ts.loss), ("pixel", ts.l1_loss), ("ssim", ts.ssim_loss), ("grad_norm", ts.grad_norm), ("clip_coef", ts.clip_coef)):
            sums[name] += float(t)
        for name, s in sums.items():
            assert r["infos"][n]["means"][name] == s / (n + 1), (n, name)
    assert sums["ssim"] > 0.0 and sums["grad_norm"] > 0.0 and r["infos"][-1]["record"]["clip_coef"]["max"] <= 1.0
    _same_state(r["state"], _state(model, ts))


def test_the_batch_loop_reads_no_device_value(tmp_path):
    model, ts, ds, valid = _objects()
    inside = [False]
    real_loader = ds.loader

    def loader(*a, **k):
        inside[0] = True
        try:
            yield from real_loader(*a, **k)
        finally:
            inside[0] = False
    ds.loader = loader
    seen = []

    def guard(name, real):
        def f(self, *a, **k):
            if inside[0] and self.is_cuda:
                seen.append(name)
                raise AssertionError(f"Tensor.{name} on a device value inside the batch loop")
            return real(self, *a, **k)
        return f
    names = ("item", "cpu", "tolist", "__float__")
    reals = {n: getattr(torch.Tensor, n) for n in names}
    for n in names:
        setattr(torch.Tensor, n, guard(n, reals[n]))
    try:
        with pytest.raises(AssertionError, match="inside the batch loop"):     # the guard itself works
            inside[0] = True
            torch.zeros(1, device="cuda").item()
        inside[0] = False
        seen.clear()
        r = _fit(tmp_path, objects=(model, ts, ds, valid), epochs=1, log_every=100, preview_every=100)
    finally:
        for n in names:
            setattr(torch.Tensor, n, reals[n])
    assert seen == [] and r["state"]["step_count"] == 3 and r["infos"] == []
    assert len(r["stat"]["mine"]["psnrs"]) == 1                                # validation and the checkpoint still read
    assert os.path.exists(tmp_path / "models" / "model_x4_1.pt")


def test_command_line_from_a_config_and_two_folders_to_a_checkpoint(tmp_path, capsys):
    """`python -m m2trans_amd.train` in process: a yaml with the reference's keys plus `training_dataset: folder` / `eval_folders`,
    then --resume of the experiment directory it made."""
    import yaml
    from PIL import Image
    from m2trans_amd import train as T
    (tmp_path / "hr").mkdir()
    (tmp_path / "val").mkdir()
    for k, im in enumerate(_images()):
        Image.fromarray(im).save(tmp_path / "hr" / f"{k}.png")
    Image.fromarray(_images()[2][:96, :128].copy()).save(tmp_path / "val" / "v.png")
    cfg = {"model": "M2Trans", "scale": SCALE, "rgb_range": 1.0, "colors": 3, "n_feats": 64, "num_heads": 4, "n_blocks": 1, "pretrain": None,
           "patch_size": PATCH, "batch_size": BATCH, "data_repeat": REPEAT, "data_augment": 1, "data_add_noise": False, "cutout": False,
           "cutmix": True, "epochs": 2, "lr": LR0, "eta_min": ETA_MIN, "gamma": 0.5, "log_every": 2, "test_every": 1,
           "log_path": str(tmp_path / "experiments"), "log_name": "run", "lambda_l1": 1.0, "lambda_clip": 0.01, "gpu_ids": [0],
           "threads": 8, "save_image": True, "training_dataset": "folder", "train_hr_path": str(tmp_path / "hr"),
           "eval_folders": {"mine": str(tmp_path / "val")}, "lambda_ssim": 0.1, "preview_every": 3}
    (tmp_path / "c.yml").write_text(yaml.dump(cfg))
    with pytest.raises(T.M2TError, match="--set lambda_clip=0"):
        T.main(["--config", str(tmp_path / "c.yml")])
    assert T.main(["--config", str(tmp_path / "c.yml"), "--compute_dtype", "fp32", "--set", "lambda_clip=0", "--set", "epochs=1"]) == 0
    (exp,) = os.listdir(tmp_path / "experiments")
    assert exp.startswith("run-20")
    exp = tmp_path / "experiments" / exp
    assert sorted(os.listdir(exp)) == ["config.yml", "log.txt", "models", "preview", "stat_dict.yml", "test_results_x4"]
    assert os.listdir(exp / "models") == ["model_x4_1.pt"] and os.listdir(exp / "test_results_x4" / "mine") == ["v.png"]
    assert Image.open(exp / "test_results_x4" / "mine" / "v.png").size == (128, 96)
    assert Image.open(exp / "preview" / "epoch0001_iter000002.png").size == (3 * PATCH, PATCH)
    saved = yaml.safe_load(open(exp / "config.yml"))
    assert saved["lambda_clip"] == 0 and saved["epochs"] == 1 and saved["lambda_ssim"] == 0.1
    text = open(exp / "log.txt").read()
    assert text == capsys.readouterr().out
    assert "accepted and ignored: gpu_ids, threads, num_heads" in text and "Epoch:1, 4/6, loss: " in text and "[mine-X4], PSNR/SSIM: " in text
    ckpt = torch.load(exp / "models" / "model_x4_1.pt", map_location="cpu", weights_only=False)
    assert ckpt["m2t_loss"]["lambda_ssim"] == 0.1 and ckpt["stat_dict"]["epochs"] == 1
    # a second session continues in the same directory, with the schedule of two epochs
    assert T.main(["--config", str(tmp_path / "c.yml"), "--compute_dtype", "fp32", "--set", "lambda_clip=0", "--resume", str(exp)]) == 0
    assert sorted(os.listdir(exp / "models")) == ["model_x4_1.pt", "model_x4_2.pt"]
    assert "resume training from epoch 2" in open(exp / "log.txt").read()
    assert yaml.safe_load(open(exp / "stat_dict.yml"))["epochs"] == 2


def test_fit_refuses_more_than_one_rank(tmp_path):
    from m2trans_amd import train as T
    model, ts, ds, valid = _objects()
    ts.world_size = 2
    with pytest.raises(T.M2TError, match="one rank"):
        T.fit(model, ts, ds, valid, epochs=1, batch_size=BATCH, lr0=LR0, eta_min=ETA_MIN, log_every=1, test_every=1, out_dir=str(tmp_path))
