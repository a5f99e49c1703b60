"""CPU tests (no GPU) of the training entry (include/m2t_train.h, m2trans_amd/train.py): the tenth header against its signature
table and the library's symbols, the argument errors of its entries, the yaml resolution of the command line, the bookkeeping of the
epoch loop (directory naming, stat_dict, checkpoint pick, learning-rate table) and the restatements of tests/train_ref.py."""
import ctypes as C
import datetime
import math
import os
import re

import numpy as np
import pytest

from tests import train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_meter_column_limit_is_the_headers():
    from m2trans_amd import _lib
    text = open(os.path.join(ROOT, "include", "m2t_train.h")).read()
    assert "#define M2T_METER_MAX_COLS 16" in text and _lib.METER_MAX_COLS == 16


def test_argument_errors_need_no_device():
    """Every M2T_ERR_ARG of the header is decided on the host before any launch, so it is reported without a device too."""
    from m2trans_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(4096)                                     # never dereferenced: the checks come first
    assert lib.m2t_meter_reset(one, one, 0, 4, None) == -2
    assert lib.m2t_meter_reset(one, one, 17, 4, None) == -2
    assert lib.m2t_meter_reset(None, one, 3, 4, None) == -2
    assert lib.m2t_meter_reset(one, one, 3, 0, None) == -2
    vals, kinds = (C.c_void_p * 17)(), (C.c_int * 17)()
    assert lib.m2t_meter_update(vals, kinds, 0, one, one, 4, 0, None) == -2
    assert lib.m2t_meter_update(vals, kinds, 17, one, one, 4, 0, None) == -2
    assert lib.m2t_meter_update(vals, kinds, 3, None, one, 4, 0, None) == -2
    assert lib.m2t_meter_update(vals, kinds, 3, one, one, 0, 0, None) == -2
    assert lib.m2t_meter_update(None, kinds, 3, one, one, 4, 0, None) == -2
    assert lib.m2t_meter_update(vals, kinds, 3, one, one, 4, -1, None) == -2
    kinds[1] = 2
    assert lib.m2t_meter_update(vals, kinds, 3, one, one, 4, 0, None) == -2
    assert b"m2t_meter_update" in lib.m2t_last_error_string()
    for scale in (1, 5, 0, -2):
        assert lib.m2t_preview_strip(one, one, one, 8, 8, scale, 1.0, one, None) == -2
    assert lib.m2t_preview_strip(one, one, one, 0, 8, 2, 1.0, one, None) == -2
    assert lib.m2t_preview_strip(one, one, one, 8, 0, 2, 1.0, one, None) == -2
    assert lib.m2t_preview_strip(one, one, one, 8, -3, 4, 1.0, one, None) == -2
    assert lib.m2t_preview_strip(None, one, one, 8, 8, 2, 1.0, one, None) == -2
    assert lib.m2t_preview_strip(one, one, one, 8, 8, 2, 0.0, one, None) == -2
    assert lib.m2t_preview_strip(one, one, one, 8192, 8, 4, 1.0, one, None) == -2
    assert b"m2t_preview_strip" in lib.m2t_last_error_string()


def test_host_tensors_are_refused():
    import torch
    from m2trans_amd import train as T
    with pytest.raises(T.M2TError):
        T.StepMeter(["loss"], "cpu")
    with pytest.raises(T.M2TError):
        T.StepMeter([], "cuda")
    with pytest.raises(T.M2TError):
        T.StepMeter([str(i) for i in range(17)], "cuda")
    with pytest.raises(T.M2TError):
        T.preview_strip(torch.zeros(3, 4, 4), torch.zeros(3, 8, 8), torch.zeros(3, 8, 8))


# ------------------------------------------------------------------------------------------------------------- the command line
REFERENCE_YAML = """
model: 'M2Trans'
scale: 4
rgb_range: 1.0
colors: 3
n_feats: 64
num_heads: 4
n_blocks: 8
pretrain:
patch_size: 384
batch_size: 2
data_repeat: 5
data_augment: 1
data_add_noise: False
cutout: False
cutmix: False
epochs: 200
lr: 0.0001
eta_min: 0.000001
gamma: 0.5
log_every: 200
test_every: 1
log_path: "./experiments"
log_name:
lambda_l1: 1.0
lambda_clip: 0.0
gpu_ids: [3]
threads: 8
save_image: True
data_path: '../SR_datasets/'
training_dataset: 'us1k'
eval_sets: ['CCA-US', 'US-CASE', 'US1K_23']
"""

EXTENSION_YAML = """
scale: 2
n_blocks: 2
compute_dtype: bf16
patch_size: 96
batch_size: 8
epochs: 10
lr: 0.0002
eta_min: 0.00001
log_every: 5
test_every: 2
cutmix: True
training_dataset: folder
train_hr_path: /data/hr
eval_folders: {mine: /data/val}
pixel_loss: charbonnier
pixel_loss_param: 0.001
lambda_ssim: 0.1
lambda_msssim: 0.0
lambda_fft: 0.05
fft_norm: ortho
lambda_vif: 0.0
accum_steps: 2
max_grad_norm: 1.0
weight_decay: 0.01
decoupled_weight_decay: True
ema_decay: 0.999
skip_nonfinite: True
param_groups: requires_grad
preview_every: 50
validate_ema: True
"""


def test_yaml_resolves_to_keyword_arguments():
    import yaml
    from m2trans_amd import train as T
    r = T.resolve_config(yaml.safe_load(REFERENCE_YAML))
    assert r["model"] == {"scale": 4, "rgb_range": 1.0, "colors": 3, "n_feats": 64, "n_blocks": 8}
    assert r["train_step"] == {"lr": 1e-4, "lambda_l1": 1.0, "lambda_clip": 0.0, "world_size": 1}
    assert r["fit"] == {"epochs": 200, "batch_size": 2, "lr0": 1e-4, "eta_min": 1e-6, "log_every": 200, "test_every": 1, "cutmix": False,
                        "cutout": False, "patch_size": 384, "save_image": True, "preview_every": 200, "validate_ema": False, "seed": 33,
                        "ring_rows": 1024}
    assert r["data"]["training_dataset"] == "us1k" and r["data"]["eval_sets"] == ["CCA-US", "US-CASE", "US1K_23"]
    assert r["data"]["data_repeat"] == 5 and r["data"]["data_augment"] is True and r["data"]["eval_folders"] == {}
    assert r["ignored"] == ["gpu_ids", "threads", "num_heads"] and r["log_name"] is None and r["log_path"] == "./experiments"
    assert T.resolve_config(yaml.safe_load(REFERENCE_YAML), "bf16")["model"]["compute_dtype"] == "bf16"

    r = T.resolve_config(yaml.safe_load(EXTENSION_YAML))
    ts = r["train_step"]
    for k, v in {"pixel_loss": "charbonnier", "pixel_loss_param": 0.001, "lambda_ssim": 0.1, "lambda_msssim": 0.0, "lambda_fft": 0.05,
                 "fft_norm": "ortho", "lambda_vif": 0.0, "accum_steps": 2, "max_grad_norm": 1.0, "weight_decay": 0.01,
                 "decoupled_weight_decay": True, "ema_decay": 0.999, "skip_nonfinite": True, "param_groups": "requires_grad"}.items():
        assert ts[k] == v and type(ts[k]) is type(v), k           # handed through unchanged: TrainStep validates them
    import inspect
    from m2trans_amd.train_step import TrainStep
    assert set(ts) <= set(inspect.signature(TrainStep.__init__).parameters)
    assert set(r["fit"]) <= set(inspect.signature(T.fit).parameters)
    assert r["fit"]["cutmix"] is True and r["fit"]["validate_ema"] is True and r["fit"]["preview_every"] == 50
    assert r["model"]["compute_dtype"] == "bf16" and r["model"]["scale"] == 2
    assert r["data"]["training_dataset"] == "folder" and r["data"]["train_hr_path"] == "/data/hr"
    assert r["data"]["eval_folders"] == {"mine": "/data/val"} and r["data"]["eval_sets"] == []


def test_unknown_keys_and_lambda_clip_are_refused():
    import yaml
    from m2trans_amd import train as T
    cfg = yaml.safe_load(REFERENCE_YAML)
    with pytest.raises(T.M2TError, match="lamda_ssim"):
        T.resolve_config(dict(cfg, lamda_ssim=0.1))
    with pytest.raises(T.M2TError, match="--set lambda_clip=0"):
        T.resolve_config(dict(cfg, lambda_clip=0.01))
    with pytest.raises(T.M2TError, match="train_hr_path"):
        T.resolve_config(dict(cfg, training_dataset="folder"))
    with pytest.raises(T.M2TError, match="epochs"):
        T.resolve_config({k: v for k, v in cfg.items() if k != "epochs"})
    assert T.resolve_config(dict(cfg, config="c.yml", resume=None))["fit"]["epochs"] == 200     # a config.yml fed back in
    over = T.apply_overrides(cfg, ["lambda_clip=0", "eval_sets=[CCA-US]", "log_name=run7", "lr=2e-4"])
    assert over["lambda_clip"] == 0 and over["eval_sets"] == ["CCA-US"] and over["log_name"] == "run7" and cfg["log_name"] is None
    with pytest.raises(T.M2TError):
        T.apply_overrides(cfg, ["lambda_clip"])
    a = T.parse_args(["--config", "c.yml", "--resume", "exp", "--compute_dtype", "bf16", "--set", "a=1", "--set", "b=2"])
    assert (a.config, a.resume, a.compute_dtype, a.set) == ("c.yml", "exp", "bf16", ["a=1", "b=2"])
    for bad in ([], ["--config", "c.yml", "--compute_dtype", "fp16"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)


def test_experiment_directory_naming():
    from m2trans_amd import train as T
    stamp = T.timestamp_str(datetime.datetime(2024, 3, 7, 9, 5))
    assert stamp == "2024-0307-0905"
    assert T.experiment_dir("./experiments", None, "M2Trans", 4, stamp) == os.path.join("./experiments", "M2Trans-fp32-x4-2024-0307-0905")
    assert T.experiment_dir("/logs", "run7", "M2Trans", 2, stamp) == os.path.join("/logs", "run7-2024-0307-0905")


# ------------------------------------------------------------------------------------------------------------- bookkeeping
def test_stat_dict_rounding_and_best_epoch_on_ties():
    from m2trans_amd import train as T
    sd = T.new_stat_dict(["CCA-US", "mine"])
    assert sd["epochs"] == 0 and sd["losses"] == [] and sd["ema_loss"] == 0.0
    assert sd["mine"] == {"psnrs": [], "ssims": [], "best_psnr": {"value": 0.0, "epoch": 0}, "best_ssim": {"value": 0.0, "epoch": 0}}
    assert T.round_scores(32.714, 0.91234) == (round(32.714 + 5e-3, 2), round(0.91234 + 5e-5, 4)) == (32.72, 0.9124)
    assert T.round_scores(30.0, 0.5) == (round(30.005, 2), round(0.50005, 4))
    line = T.update_stats(sd, "mine", 30.5, 0.9, 1, 4)
    assert line == "[mine-X4], PSNR/SSIM: 30.5000/0.9000 (Best: 30.5000/0.9000, Epoch: 1/1)\n"
    T.update_stats(sd, "mine", 30.5, 0.95, 2, 4)                # a tie on PSNR keeps epoch 1, SSIM improves
    assert sd["mine"]["best_psnr"] == {"value": 30.5, "epoch": 1} and sd["mine"]["best_ssim"] == {"value": 0.95, "epoch": 2}
    line = T.update_stats(sd, "mine", 29.0, 0.95, 3, 4)
    assert sd["mine"]["best_psnr"]["epoch"] == 1 and sd["mine"]["best_ssim"]["epoch"] == 2
    assert sd["mine"]["psnrs"] == [30.5, 30.5, 29.0] and sd["mine"]["ssims"] == [0.9, 0.95, 0.95]
    assert line == "[mine-X4], PSNR/SSIM: 29.0000/0.9500 (Best: 30.5000/0.9500, Epoch: 1/2)\n"
    assert sd["CCA-US"]["psnrs"] == []


def test_the_checkpoint_pick_is_numeric(tmp_path):
    from m2trans_amd import train as T
    assert T.latest_checkpoint(tmp_path) is None
    (tmp_path / "models").mkdir()
    assert T.latest_checkpoint(tmp_path) is None
    for n in ("model_x4_2.pt", "model_x4_10.pt", "model_x4_9.pt"):
        (tmp_path / "models" / n).write_bytes(b"")
    assert sorted(os.listdir(tmp_path / "models"))[-1] == "model_x4_9.pt"      # what a lexical order would pick
    assert os.path.basename(T.latest_checkpoint(tmp_path)) == "model_x4_10.pt"


def test_epoch_to_rate_table():
    from m2trans_amd import train as T
    from m2trans_amd.train_step import cosine_lr
    lr0, eta, E = 1e-4, 1e-6, 200
    table = T.epoch_rates(1, E, lr0, eta)
    assert list(table) == list(range(1, E + 1))
    assert all(table[e] == cosine_lr(e - 1, lr0, eta, E) for e in table)
    assert table[1] == lr0 and table[E] > eta
    assert table[101] == pytest.approx(eta + 0.5 * (lr0 - eta) * (1 + math.cos(math.pi * 100 / 200)))
    # a run continued from one of its own checkpoints (saved after epoch 7) continues the table
    cont = T.epoch_rates(8, E, lr0, eta)
    assert cont == {e: table[e] for e in range(8, E + 1)}
    # a file of the reference, resumed the reference's way: epoch 8 re-uses the rate epoch 7 trained with and the schedule stays
    # one step behind from there on (the saved scheduler has last_epoch = 6; train.py:101-103,358)
    saved = cosine_lr(6, lr0, eta, E)
    ref = T.epoch_rates(8, E, lr0, eta, resumed_lr=saved)
    assert ref[8] == saved == table[7] and ref[9] == table[8] and ref[E] == table[E - 1]


def test_rng_state_round_trip_is_plain_data():
    import pickle
    import random
    import torch
    from m2trans_amd import train as T
    g = torch.Generator()
    g.manual_seed(5)
    random.seed(5), np.random.seed(5), torch.manual_seed(5)
    np.random.normal()                                          # (leaves a cached gaussian in the legacy state)
    state = pickle.loads(pickle.dumps(T.rng_state(g)))

    def plain(o):
        return all(plain(v) for v in o) if isinstance(o, (list, tuple)) else \
            all(isinstance(k, str) and plain(v) for k, v in o.items()) if isinstance(o, dict) else isinstance(o, (int, float, str, type(None)))
    assert plain(state) and set(state) == {"random", "numpy", "torch", "loader"}
    want = (random.random(), np.random.randint(1, 5), np.random.normal(), torch.randperm(7).tolist(), torch.randperm(9, generator=g).tolist())
    random.seed(1), np.random.seed(1), torch.manual_seed(1), g.manual_seed(1)
    T.set_rng_state(state, g)
    got = (random.random(), np.random.randint(1, 5), np.random.normal(), torch.randperm(7).tolist(), torch.randperm(9, generator=g).tolist())
    assert got == want


def test_meter_columns_follow_the_terms_that_are_on():
    import types
    from m2trans_amd import train as T
    off = types.SimpleNamespace()
    assert T.meter_columns(off) == ["loss", "pixel", "clip"]
    on = types.SimpleNamespace(lambda_ssim=0.1, lambda_vif=0.2, lambda_fft=0.0, lambda_perceptual=0.5, grad_norm=object())
    assert T.meter_columns(on) == ["loss", "pixel", "clip", "ssim", "vif", "perceptual", "grad_norm", "clip_coef"]


# ------------------------------------------------------------------------------------------------------------- the restatements
def test_the_restated_meter_keeps_sum_counts_extremes_and_ring():
    m = R.RefMeter(2, 3)
    assert m.record[0].tolist() == [0, 0, 0, math.inf, -math.inf, 0, 0, 0] and np.isnan(m.ring).all()
    seq = [0.1, 0.2, float("nan"), 0.3, float("inf"), -0.4]
    s = 0.0
    for step, v in enumerate(seq):
        m.update([v, None], step)
        if math.isfinite(v):
            s += v
    assert m.record[0, :5].tolist() == [s, 4.0, 2.0, -0.4, 0.3] and m.record[0, 5] == -0.4
    assert m.record[1].tolist() == [0, 0, 0, math.inf, -math.inf, 0, 0, 0]
    assert m.ring[:, 0].tolist() == [3.0, 4.0, 5.0] and np.isnan(m.ring[:, 2]).all()        # wrapped once
    assert m.ring[0, 1] == np.float32(0.3) and np.isinf(m.ring[1, 1]) and m.ring[2, 1] == np.float32(-0.4)


def test_the_restated_preview_on_a_hand_worked_2x2_at_x2():
    # one channel of interest (the others constant): q = [[0, 255], [100, 40]] at rgb_range 255
    q = np.array([[0.0, 255.0], [100.0, 40.0]], dtype=np.float32)
    lr = np.stack([q, np.full((2, 2), 7.9, np.float32), np.full((2, 2), -3.0, np.float32)])
    sr = np.zeros((3, 4, 4), np.float32)
    hr = np.full((3, 4, 4), 254.999, np.float32)
    sr[0, 0, 0], sr[1, 0, 0], sr[2, 0, 0], sr[0, 3, 3] = 127.99, float("nan"), 300.0, 255.0
    out = R.preview_strip(lr, sr, hr, 255.0)
    assert out.shape == (4, 12, 3) and out.dtype == np.uint8
    # per axis the weights out of 4 are (4,0) (3,1) (1,3) (0,4): rows / columns 0 and 3 are the source's own
    a, b, c, d = 0, 255, 100, 40
    want = np.array([[a, (3 * a + b) * 4, (a + 3 * b) * 4, b * 16],
                     [(3 * a + c) * 4, 9 * a + 3 * b + 3 * c + d, 3 * a + 9 * b + c + 3 * d, (3 * b + d) * 4],
                     [(a + 3 * c) * 4, 3 * a + b + 9 * c + 3 * d, a + 3 * b + 3 * c + 9 * d, (b + 3 * d) * 4],
                     [c * 16, (3 * c + d) * 16 // 4, (c + 3 * d) * 16 // 4, d * 16]])
    want[0, 0] = a * 16
    want = (want + 8) // 16
    assert want[1].tolist() == [25, 69, 157, 201] and want[0].tolist() == [0, 64, 191, 255] and want[3].tolist() == [100, 85, 55, 40]
    assert out[:, :4, 0].tolist() == want.tolist()
    assert (out[:, :4, 1] == 7).all() and (out[:, :4, 2] == 0).all()                 # truncation, clamp below
    assert out[0, 4].tolist() == [127, 0, 255] and out[3, 7, 0] == 255 and out[1, 5].tolist() == [0, 0, 0]
    assert (out[:, 8:] == 254).all()                                                 # 254.999 truncates: not save_image's rounding
    # rgb_range 1.0: exactly the range is 255, just below it is 254
    one = np.full((3, 2, 2), 1.0, np.float32)
    o = R.preview_strip(one, np.full((3, 4, 4), np.float32(1.0) - np.float32(2.0 ** -24), np.float32), np.full((3, 4, 4), 1.7, np.float32), 1.0)
    assert (o[:, :4] == 255).all() and (o[:, 4:8] == 254).all() and (o[:, 8:] == 255).all()


@pytest.mark.parametrize("s", [2, 3, 4])
def test_the_restated_upsampling_keeps_constants_and_stays_between_its_taps(s):
    rng = np.random.RandomState(s)
    q = rng.randint(0, 256, size=(3, 5, 7)).astype(np.int64)
    up = R.upsample_quantised(q, s)
    assert up.shape == (3, 5 * s, 7 * s) and up.min() >= q.min() and up.max() <= q.max()
    assert (R.upsample_quantised(np.full((3, 5, 7), 200, np.int64), s) == 200).all()
    # the corners are the source's corners (clamped borders), and flipping the source flips the result (half-pixel centres)
    assert (up[:, 0, 0] == q[:, 0, 0]).all() and (up[:, -1, -1] == q[:, -1, -1]).all()
    assert (R.upsample_quantised(q[:, ::-1, ::-1], s) == up[:, ::-1, ::-1]).all()
