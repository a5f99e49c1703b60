"""The training entry (include/m2t_train.h, k_train.hip): the reference's epoch loop (train.py:160-358) on `TrainStep`, from a config
file and a data folder to `models/model_x<scale>_<epoch>.pt`.

    python -m m2trans_amd.train --config configs/M2Trans_x4.yml [--resume DIR] [--compute_dtype bf16|fp32] [--set key=value ...]

`fit` is the loop: batches from `datas.US1K.loader`, cutmix / cutout (augment.py), `TrainStep.step`, logging, the preview image,
validation through `metrics.evaluate`, `stat_dict`, checkpoints (checkpoint.py) and resume.  Two things differ from the reference
on the timed path.  The reference reads `float(loss)` three times per step (train.py:212-214); here the per-step values go into a
device-resident meter (`StepMeter`: one m2t_meter_update launch per step) that the host reads once per `log_every`.  The reference
builds its "LR upsampled | SR | HR" preview on the host with numpy and cv2 (train.py:218-233); here one kernel (m2t_preview_strip)
builds it on the device.  Inside the batch loop nothing reads a device value.

Device tensors only: there is no host fallback.  One rank only; TensorBoard and the complexity printing of the reference are not
built (the meter's ring buffer and the preview PNGs stand in for the former)."""
from __future__ import annotations

import ctypes as C
import datetime
import glob
import math
import os
import random
import sys
import time
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, augment
from ._lib import M2TError
from .train_step import LOSS_TERMS, cosine_lr

EVAL_SETS = {"CCA-US": "UI5", "US-CASE": "US15", "US1K_23": "US1K_23"}        # datas/utils.py:27-43: name -> benchmark/<folder>


# ------------------------------------------------------------------------------------------------------------------ the meter
class StepMeter:
    """The per-step scalars of a run, kept on the device (include/m2t_train.h): per column sum / count / nonfinite / min / max /
    last in fp64, and a float32 ring [ring_rows, n_cols + 1] of the last `ring_rows` steps (step index first).  `update` is one
    launch and no synchronisation; `read` and `curves` are the caller's synchronisation, at the caller's cadence."""

    def __init__(self, names, device, ring_rows: int = 1024):
        self.names = list(names)
        n = len(self.names)
        if not 1 <= n <= _lib.METER_MAX_COLS:
            raise M2TError(f"StepMeter takes 1 .. {_lib.METER_MAX_COLS} columns, got {n}: {self.names}")
        if int(ring_rows) < 1:
            raise M2TError(f"ring_rows must be >= 1, got {ring_rows!r}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise M2TError("StepMeter keeps its record on the device: a HIP device is required")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.ring_rows = int(ring_rows)
        self.record = torch.empty(n, 8, dtype=torch.float64, device=self.device)
        self.ring = torch.empty(self.ring_rows, n + 1, dtype=torch.float32, device=self.device)
        self.reset()

    def reset(self):
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().m2t_meter_reset(_lib.ptr(self.record), _lib.ptr(self.ring), len(self.names), self.ring_rows,
                                                   _lib.stream_ptr()), "m2t_meter_reset")

    def update(self, values, step: int):
        """values: per column a one-element float32 / float64 device tensor, or None for a column that is absent this step."""
        n = len(self.names)
        if len(values) != n:
            raise M2TError(f"StepMeter.update: {n} columns, {len(values)} values")
        ptrs, kinds = (C.c_void_p * n)(), (C.c_int * n)()
        for c, v in enumerate(values):
            if v is None:
                continue
            if not isinstance(v, torch.Tensor) or v.numel() != 1 or v.device != self.device or v.dtype not in (torch.float32, torch.float64):
                got = f"{v.dtype} {tuple(v.shape)} on {v.device}" if isinstance(v, torch.Tensor) else type(v).__name__
                raise M2TError(f"StepMeter.update: column {self.names[c]!r} must be a one-element float32 / float64 tensor on "
                               f"{self.device}, got {got}")
            ptrs[c] = v.data_ptr()
            kinds[c] = 1 if v.dtype == torch.float64 else 0
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().m2t_meter_update(ptrs, kinds, n, _lib.ptr(self.record), _lib.ptr(self.ring), self.ring_rows,
                                                    int(step), _lib.stream_ptr()), "m2t_meter_update")

    def read(self) -> Dict[str, Dict[str, float]]:
        """{column: {sum, count, nonfinite, min, max, last}} as Python floats.  One device-to-host copy: synchronises."""
        rec = self.record.cpu()
        return {name: {k: float(rec[c, i]) for i, k in enumerate(_lib.METER_RECORD)} for c, name in enumerate(self.names)}

    def curves(self) -> torch.Tensor:
        """The ring on the host, its rows sorted by step index (rows never written are dropped).  Synchronises."""
        ring = self.ring.cpu()
        ring = ring[~torch.isnan(ring[:, 0])]
        return ring[torch.argsort(ring[:, 0])]


def meter_columns(train_step) -> List[str]:
    """The columns `fit` meters for this step object: the total loss, the pixel term, the clip term, every optional term that is on
    (LOSS_TERMS, then the perceptual term) and, when the step tracks them, the gradient norm and the clip coefficient."""
    names = ["loss", "pixel", "clip"] + [t.name for t in LOSS_TERMS if getattr(train_step, f"lambda_{t.name}", 0.0) > 0.0]
    if getattr(train_step, "lambda_perceptual", 0.0) > 0.0:
        names.append("perceptual")
    if getattr(train_step, "grad_norm", None) is not None:
        names += ["grad_norm", "clip_coef"]
    return names


def meter_values(train_step, names) -> list:
    """The device scalars behind `meter_columns`, after a step: tensors the step object owns, never copies."""
    where = {"loss": train_step.loss, "pixel": train_step.l1_loss, "clip": train_step.clip_loss,
             "perceptual": getattr(train_step, "perceptual_loss_value", None),
             "grad_norm": getattr(train_step, "grad_norm", None), "clip_coef": getattr(train_step, "clip_coef", None)}
    return [where[n] if n in where else getattr(train_step, f"{n}_loss") for n in names]


# ------------------------------------------------------------------------------------------------------------------ the preview
def preview_strip(lr: torch.Tensor, sr: torch.Tensor, hr: torch.Tensor, rgb_range: float = 1.0) -> torch.Tensor:
    """One sample, lr [3,h,w] and sr, hr [3,h*s,w*s] float32 on the device (s = 2, 3 or 4) -> uint8 [h*s, 3*w*s, 3] on the device:
    the bilinearly upsampled LR, SR and HR side by side, quantised by truncation (include/m2t_train.h).  One launch."""
    for name, t in (("lr", lr), ("sr", sr), ("hr", hr)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != 3 or not t.is_cuda:
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise M2TError(f"preview_strip: {name} must be a float32 [3,H,W] device tensor, got {got}")
    _, h, w = lr.shape
    s = sr.shape[1] // h if h else 0
    if tuple(sr.shape) != (3, h * s, w * s) or tuple(hr.shape) != tuple(sr.shape) or sr.device != lr.device or hr.device != lr.device:
        raise M2TError(f"preview_strip: sr and hr must be [3,h*s,w*s] for lr [3,{h},{w}] on one device, got {tuple(sr.shape)} and "
                       f"{tuple(hr.shape)}")
    lr, sr, hr = lr.detach().contiguous(), sr.detach().contiguous(), hr.detach().contiguous()
    out = torch.empty(h * s, 3 * w * s, 3, dtype=torch.uint8, device=lr.device)
    with torch.cuda.device(lr.device):
        _lib.check(_lib.load().m2t_preview_strip(_lib.ptr(lr), _lib.ptr(sr), _lib.ptr(hr), h, w, s, float(rgb_range), _lib.ptr(out),
                                                 _lib.stream_ptr()), "m2t_preview_strip")
    return out


# ------------------------------------------------------------------------------------------------------------------ bookkeeping
def new_stat_dict(names) -> dict:
    """utils.get_stat_dict() for the evaluation sets `names`."""
    out = {"epochs": 0, "losses": [], "ema_loss": 0.0}
    for n in names:
        out[n] = {"psnrs": [], "ssims": [], "best_psnr": {"value": 0.0, "epoch": 0}, "best_ssim": {"value": 0.0, "epoch": 0}}
    return out


def round_scores(psnr_mean: float, ssim_mean: float):
    """train.py:316-317: the rounding of the per-set averages (what metrics.evaluate applies to the means it returns)."""
    return round(psnr_mean + 5e-3, 2), round(ssim_mean + 5e-5, 4)


def update_stats(stat_dict: dict, name: str, avg_psnr: float, avg_ssim: float, epoch: int, scale: int) -> str:
    """train.py:323-335 for one evaluation set (scores already rounded): append, move the best values on a strict improvement only
    (a tie keeps the earlier epoch), return the set's log line."""
    s = stat_dict.setdefault(name, new_stat_dict([name])[name])
    s["psnrs"].append(avg_psnr)
    s["ssims"].append(avg_ssim)
    if s["best_psnr"]["value"] < avg_psnr:
        s["best_psnr"]["value"], s["best_psnr"]["epoch"] = avg_psnr, epoch
    if s["best_ssim"]["value"] < avg_ssim:
        s["best_ssim"]["value"], s["best_ssim"]["epoch"] = avg_ssim, epoch
    return "[{}-X{}], PSNR/SSIM: {:.4f}/{:.4f} (Best: {:.4f}/{:.4f}, Epoch: {}/{})\n".format(
        name, scale, float(avg_psnr), float(avg_ssim), s["best_psnr"]["value"], s["best_ssim"]["value"], s["best_psnr"]["epoch"],
        s["best_ssim"]["epoch"])


def latest_checkpoint(resume_dir) -> Optional[str]:
    """train.py:93-96: the checkpoint of `<resume_dir>/models/*.pt` with the highest trailing number (numeric order), or None."""
    files = glob.glob(os.path.join(str(resume_dir), "models", "*.pt"))
    if not files:
        return None
    return sorted(files, key=lambda x: int(x.replace(".pt", "").split("_")[-1]))[-1]


def epoch_rates(start_epoch: int, epochs: int, lr0: float, eta_min: float, resumed_lr: Optional[float] = None) -> Dict[int, float]:
    """{epoch: learning rate} of the epochs start_epoch .. epochs (1-based).  A run from its own start, and a resumed run that
    continues exactly (`resumed_lr=None`), trains epoch e at cosine_lr(e - 1).  With `resumed_lr` (the rate the optimizer state of
    a checkpoint carries) the table is the reference's after `--resume` (train.py:101-103,358): the first epoch re-uses the saved
    rate, the scheduler having been restored to last_epoch = start_epoch - 2, and every later epoch e runs at cosine_lr(e - 2)."""
    if resumed_lr is None:
        return {e: cosine_lr(e - 1, lr0, eta_min, epochs) for e in range(start_epoch, epochs + 1)}
    return {e: float(resumed_lr) if e == start_epoch else cosine_lr(e - 2, lr0, eta_min, epochs) for e in range(start_epoch, epochs + 1)}


def rng_state(generator: torch.Generator) -> dict:
    """The four generators the loop draws from, as plain picklable data (the checkpoint's ``m2t_rng`` entry)."""
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return {"random": random.getstate(), "numpy": (str(kind), keys.tolist(), int(pos), int(has_gauss), float(cached)),
            "torch": torch.get_rng_state().tolist(), "loader": generator.get_state().tolist()}


def set_rng_state(state: dict, generator: torch.Generator) -> None:
    r = state["random"]
    random.setstate((r[0], tuple(r[1]), r[2]))
    kind, keys, pos, has_gauss, cached = state["numpy"]
    np.random.set_state((kind, np.asarray(keys, dtype=np.uint32), pos, has_gauss, cached))
    torch.set_rng_state(torch.tensor(state["torch"], dtype=torch.uint8))
    generator.set_state(torch.tensor(state["loader"], dtype=torch.uint8))


def _valid_sets(valid_sets) -> list:
    if valid_sets is None:
        return []
    return list(valid_sets.items()) if isinstance(valid_sets, dict) else [(n, s) for n, s in valid_sets]


# ------------------------------------------------------------------------------------------------------------------ the loop
def run_epoch(model, train_step, train_set, meter, names, *, epoch, epochs, batch_size, generator, first_step=0, cutmix=False,
              cutout=False, patch_size=None, captions=None, preview_every=200, preview_dir=None, log_every=200, at_log=None) -> int:
    """The batch loop of one epoch (train.py:173-256): launches only -- no .item(), float() or .cpu() on a device value -- except
    at the two cadences: `at_log(it)` every `log_every` batches and the preview PNG every `preview_every`.  Returns the number of
    batches."""
    scale, rgb_range = int(model.scale), float(model.rgb_range)
    patch_size = int(train_set.patch_size if patch_size is None else patch_size)
    it = -1
    for it, (lr, hr) in enumerate(train_set.loader(batch_size, shuffle=True, generator=generator)):
        if cutmix:
            lr, hr = augment.cutmix(lr, hr, 1.0, np.random.randint(1, 5), scale)
        if cutout and epoch < epochs * 0.2:
            lr = augment.cut_out(lr, np.random.randint(1, 10), int(0.1 * patch_size // scale))
        B = lr.shape[0]
        batch_tokens = [captions[(it * B + i) % len(captions)] for i in range(B)] if captions else None   # train.py:190-193
        train_step.step(lr, hr, batch_tokens)
        meter.update(meter_values(train_step, names), first_step + it)
        if preview_dir is not None and (it + 1) % preview_every == 0:
            _write_preview(model, lr, hr, rgb_range, preview_dir, epoch, it)
        if at_log is not None and (it + 1) % log_every == 0:
            at_log(it)
    return it + 1


def fit(model, train_step, train_set, valid_sets, *, epochs, batch_size, lr0, eta_min, log_every, test_every, out_dir,
        cutmix=False, cutout=False, patch_size=None, captions=None, save_image=False, preview_every=200, validate_ema=False,
        resume=None, seed=33, ring_rows=1024, log=print, on_log=None, last_epoch=None):
    """The epoch loop of train.py:160-358.  `train_set`: a datas.US1K; `valid_sets`: [(name, datas.Benchmark)] or a dict;
    `out_dir`: the experiment directory (models/, preview/, test_results_x<scale>/, stat_dict.yml are written under it);
    `resume`: an experiment directory whose highest-numbered checkpoint the run continues from (out_dir may be the same).
    `on_log(info)` (optional) is called at every log point with {"epoch", "iter", "means": {column: sum / (iter + 1)}, "record":
    StepMeter.read(), "meter": the StepMeter, whose curves() are the per-step values since the epoch began}; `last_epoch`
    (optional) ends the run after that epoch with the schedule still that of `epochs` -- a time-boxed session that a later
    `resume` continues.  Returns stat_dict."""
    from .checkpoint import export_checkpoint, import_checkpoint
    from .metrics import evaluate
    if getattr(train_step, "world_size", 1) > 1:
        raise M2TError(f"fit drives one rank; this TrainStep has world_size = {train_step.world_size}")
    if int(log_every) < 1 or int(test_every) < 1 or int(preview_every) < 1 or int(epochs) < 1 or int(batch_size) < 1:
        raise M2TError("fit: epochs, batch_size, log_every, test_every and preview_every must be integers >= 1")
    if train_step.model is not model:
        raise M2TError("fit: train_step was built for another model")
    scale, rgb_range = int(model.scale), float(model.rgb_range)
    patch_size = int(train_set.patch_size if patch_size is None else patch_size)
    valid = _valid_sets(valid_sets)
    device = model.flat_params.device
    out_dir = str(out_dir)
    model_dir = os.path.join(out_dir, "models")
    os.makedirs(model_dir, exist_ok=True)

    # train.py:40-43; one generator of its own for the loader's permutation
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    generator = torch.Generator()
    generator.manual_seed(seed)

    stat_dict = new_stat_dict([n for n, _ in valid])
    start_epoch, resumed_lr = 1, None
    degradation = getattr(train_set, "degradation", None)       # its own generator: the per-sample kernel and noise draws
    if resume is not None:
        path = latest_checkpoint(resume)
        if path is not None:
            ckpt = torch.load(path, map_location="cpu", weights_only=False)
            start_epoch = import_checkpoint(ckpt, model, train_step)
            stat_dict = ckpt.get("stat_dict") or stat_dict
            log("## select {}, resume training from epoch {}. ##".format(path, start_epoch))
            if ckpt.get("m2t_rng") is not None:
                set_rng_state(ckpt["m2t_rng"], generator)       # the run continues exactly: draws and schedule
                if degradation is not None and ckpt["m2t_rng"].get("degradation") is not None:
                    degradation.set_state(ckpt["m2t_rng"]["degradation"])
                train_step.scheduler_last_epoch = start_epoch - 1
            else:
                # a file of the reference: its own resume re-uses the saved rate for the first epoch (epoch_rates)
                resumed_lr = train_step.lr
                log(f"## {path} carries no m2t_rng entry: the random draws continue from seed {seed}, not from where the saved run "
                    "stood ##")
        else:
            log(f"## no checkpoint under {os.path.join(str(resume), 'models')}: training from epoch 1 ##")
    rates = epoch_rates(start_epoch, int(epochs), float(lr0), float(eta_min), resumed_lr)

    names = meter_columns(train_step)
    meter = StepMeter(names, device, ring_rows)
    total_steps = len(train_set)
    fill_width = math.ceil(math.log10(total_steps)) if total_steps > 1 else 1
    epoch_width = math.ceil(math.log10(epochs)) if epochs > 1 else 1
    n_batches = (total_steps + batch_size - 1) // batch_size
    timer_start = time.time()
    for epoch in range(start_epoch, int(epochs) + 1):
        stat_dict["epochs"] = epoch
        model.train()
        train_step.set_lr(rates[epoch])
        log("## =========== {}-training, Epoch: {}, lr: {} ============= ##".format(model.compute_dtype, epoch, [train_step.lr]))
        meter.reset()

        def at_log(it):
            nonlocal timer_start
            rec = meter.read()                                  # the one synchronisation of a log interval
            means = {n: rec[n]["sum"] / (it + 1) for n in names}
            # train.py:244-248 divides the running mean by (iter + 1) a second time before it appends: the reference's, kept
            stat_dict["losses"].append(means["loss"] / (it + 1))
            now = time.time()
            duration, timer_start = now - timer_start, now
            log("Epoch:{}, {}/{}, loss: {:.4f}, L1loss: {:.4f}, CLIPloss: {:.8f} time: {:.3f}".format(
                str(epoch).zfill(epoch_width), str((it + 1) * batch_size).zfill(fill_width), total_steps, means["loss"],
                means["pixel"], means["clip"], duration))
            # track_health: K: the stage where a NaN / Inf first appeared in the last recorded step, else its three largest ranges
            if getattr(train_step, "track_health", 0) and getattr(train_step, "_last_plan", None) is not None:
                log(train_step.health().log_line())
            if on_log is not None:
                on_log({"epoch": epoch, "iter": it, "means": means, "record": rec, "meter": meter})

        run_epoch(model, train_step, train_set, meter, names, epoch=epoch, epochs=int(epochs), batch_size=batch_size,
                  generator=generator, first_step=(epoch - 1) * n_batches, cutmix=cutmix, cutout=cutout, patch_size=patch_size,
                  captions=captions, preview_every=preview_every, preview_dir=os.path.join(out_dir, "preview"),
                  log_every=log_every, at_log=at_log)
        # ---- validation, stat_dict, checkpoint (train.py:258-356)
        if epoch % test_every == 0:
            model.eval()
            log("## validation ##")
            test_log = ""
            if validate_ema:
                train_step.swap_ema()
            try:
                for name, bench in valid:
                    psnr, ssim = _validate(model, bench, scale, rgb_range, evaluate,
                                           os.path.join(out_dir, "test_results_x" + str(scale), name) if save_image else None)
                    test_log += update_stats(stat_dict, name, psnr, ssim, epoch, scale)
            finally:
                if validate_ema:
                    train_step.swap_ema()
            log(test_log)
            ckpt = export_checkpoint(model, train_step, epoch=epoch, stat_dict=stat_dict, lr0=float(lr0), eta_min=float(eta_min),
                                     t_max=float(epochs))
            ckpt["m2t_rng"] = rng_state(generator)
            if degradation is not None:
                ckpt["m2t_rng"]["degradation"] = degradation.get_state()
            torch.save(ckpt, os.path.join(model_dir, "model_x{}_{}.pt".format(scale, epoch)))
            _dump_yaml(stat_dict, os.path.join(out_dir, "stat_dict.yml"))
        train_step.scheduler_last_epoch += 1                    # scheduler.step(), train.py:358
        if last_epoch is not None and epoch >= int(last_epoch):
            break
    return stat_dict


def _write_preview(model, lr, hr, rgb_range, folder, epoch, it):
    """The preview of sample 0 (train.py:218-233): SR of the weights as they stand, the strip on the device, a PNG through PIL.
    The copy of the finished bytes to the host is the only read, every `preview_every` batches."""
    from PIL import Image
    with torch.no_grad():
        sr = model(lr[:1].contiguous())
    strip = preview_strip(lr[0], sr[0].float(), hr[0], rgb_range)
    os.makedirs(folder, exist_ok=True)
    Image.fromarray(strip.cpu().numpy()).save(os.path.join(folder, "epoch{:04d}_iter{:06d}.png".format(epoch, it)))


def _validate(model, bench, scale, rgb_range, evaluate, image_dir):
    """One evaluation set (train.py:264-317): (avg_psnr, avg_ssim) rounded as the reference rounds them; with image_dir every SR is
    written there under the image's own name."""
    if image_dir is None:
        out = evaluate(model, ((lr, hr) for lr, hr, _ in bench), scale, rgb_range)
        return out[0], out[1]
    from .infer import save_image as save
    os.makedirs(image_dir, exist_ok=True)
    names = iter(bench.img_name)

    def saving(x):
        sr = model(x)
        save(sr, os.path.join(image_dir, next(names)), rgb_range)      # train.py:275-278
        return sr

    out = evaluate(saving, ((lr, hr) for lr, hr, _ in bench), scale, rgb_range)
    return out[0], out[1]


def _dump_yaml(obj, path):
    import yaml
    with open(path, "w") as f:
        yaml.dump(obj, f, default_flow_style=False)


# ------------------------------------------------------------------------------------------------------------------------- CLI
# the reference's yaml keys (configs/M2Trans_x*.yml) ...
MODEL_KEYS = ("model", "scale", "rgb_range", "colors", "n_feats", "n_blocks", "compute_dtype", "lean_inference", "local_norm")
REFERENCE_KEYS = MODEL_KEYS + ("pretrain", "patch_size", "batch_size", "data_repeat", "data_augment", "data_add_noise", "cutout", "cutmix",
                               "epochs", "lr", "eta_min", "gamma", "log_every", "test_every", "log_path", "log_name", "lambda_l1",
                               "lambda_clip", "save_image", "data_path", "training_dataset", "eval_sets")
IGNORED_KEYS = ("gpu_ids", "threads", "num_heads")
# ... and the project's own, each handed to TrainStep unchanged (TrainStep validates them)
TRAINSTEP_KEYS = ("pixel_loss", "pixel_loss_param", "lambda_ssim", "lambda_msssim", "lambda_fft", "fft_norm", "lambda_vif", "lambda_gmsd", "lambda_wavelet",
                  "wavelet", "wavelet_levels", "wavelet_band_weights", "wavelet_eps", "lambda_consistency", "consistency_eps", "accum_steps",
                  "max_grad_norm", "weight_decay", "decoupled_weight_decay", "ema_decay", "skip_nonfinite", "param_groups", "track_health")
LOOP_KEYS = ("train_hr_path", "eval_folders", "preview_every", "validate_ema", "seed", "ring_rows", "track_grad_norm")
DATA_KEYS = ("degradation",)            # a mapping of degrade.Degradation's arguments: LR synthesis beyond bicubic
CLI_KEYS = ("config", "resume")         # the command line's own arguments, which config.yml records as the reference's does


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m m2trans_amd.train", description="Train M2Trans: the reference's epoch loop on TrainStep.")
    ap.add_argument("--config", required=True, help="a yaml with the reference's keys (configs/M2Trans_x*.yml) and the project's own")
    ap.add_argument("--resume", default=None, metavar="DIR", help="an experiment directory: continue from its highest-numbered checkpoint")
    ap.add_argument("--compute_dtype", choices=("bf16", "fp32"), default=None, help="overrides the yaml's compute_dtype")
    ap.add_argument("--set", action="append", default=[], metavar="key=value", help="override one yaml key (the value is parsed as yaml)")
    return ap.parse_args(argv)


def apply_overrides(cfg: dict, pairs) -> dict:
    import yaml
    out = dict(cfg)
    for p in pairs:
        if "=" not in p:
            raise M2TError(f"--set takes key=value, got {p!r}")
        k, v = p.split("=", 1)
        out[k.strip()] = yaml.safe_load(v)
    return out


def resolve_config(cfg: dict, compute_dtype=None) -> dict:
    """A yaml dictionary -> {"model": the namespace dict for infer.model_namespace, "train_step": TrainStep's keyword arguments,
    "fit": fit's keyword arguments (without out_dir / resume), "data": what build_datasets needs, "ignored": the accepted keys
    that do nothing here}.  An unknown key is an M2TError that names it."""
    known = set(REFERENCE_KEYS) | set(IGNORED_KEYS) | set(TRAINSTEP_KEYS) | set(LOOP_KEYS) | set(DATA_KEYS) | set(CLI_KEYS)
    unknown = sorted(k for k in cfg if k not in known)
    if unknown:
        raise M2TError(f"unknown config key{'s' if len(unknown) > 1 else ''}: {', '.join(unknown)}")
    for k in ("scale", "patch_size", "batch_size", "epochs", "lr", "eta_min", "log_every", "test_every"):
        if cfg.get(k) is None:
            raise M2TError(f"config key {k!r} is missing")
    if str(cfg.get("model", "M2Trans")) != "M2Trans":
        raise M2TError(f"model must be 'M2Trans', got {cfg.get('model')!r}")
    if float(cfg.get("lambda_clip") or 0.0) > 0.0:
        raise M2TError("lambda_clip > 0 needs a SemanticLoss with MedCLIP weights, and none ship: the command line cannot build one "
                       "(pass --set lambda_clip=0, or call m2trans_amd.train.fit with a TrainStep(semantic_loss=...) of your own)")
    if cfg.get("data_add_noise"):
        raise M2TError("data_add_noise is dead code in the reference (datas/us1k.py:156-167) and is not built")
    degradation = None
    if cfg.get("degradation") is not None:
        from .degrade import check_config
        degradation = check_config(cfg["degradation"])
        if float(cfg.get("lambda_consistency") or 0.0) > 0.0:
            raise M2TError("lambda_consistency > 0 together with degradation: the consistency term's operator is the bicubic down-sampler, "
                           "not the degradation's per-sample blur kernels (drop one of the two keys)")
    model = {k: cfg[k] for k in MODEL_KEYS if k in cfg and k != "model"}
    model.setdefault("n_feats", 64)
    model.setdefault("n_blocks", 8)
    model.setdefault("rgb_range", 1.0)
    model.setdefault("colors", 3)
    if compute_dtype is not None:
        model["compute_dtype"] = compute_dtype
    if "lean_inference" in model:            # validation forwards on inference plans (M2Trans.lean_inference); training plans stay cached
        if not isinstance(model["lean_inference"], bool):
            raise M2TError(f"lean_inference must be true or false, got {model['lean_inference']!r}")
    if "local_norm" in model:                # ... with local-window InstanceNorm statistics (M2Trans.local_norm): train global, test local
        T = model["local_norm"]
        if isinstance(T, bool) or not isinstance(T, int) or not (T == 0 or 8 <= T <= 16384):
            raise M2TError(f"local_norm must be 0 (off) or a window side of 8 .. 16384, got {T!r}")
    ts = {"lr": float(cfg["lr"]), "lambda_l1": float(cfg.get("lambda_l1", 1.0)), "lambda_clip": 0.0, "world_size": 1}
    ts.update({k: cfg[k] for k in TRAINSTEP_KEYS if k in cfg})
    if "track_health" in ts:                 # the step health record every K-th step (TrainStep(track_health=K)); 0 = off
        K = ts["track_health"]
        if isinstance(K, bool) or not isinstance(K, int) or K < 0:
            raise M2TError(f"track_health must be an integer >= 0 (record every K-th step; 0 = off), got {K!r}")
    if "track_grad_norm" in cfg:
        ts["track_grad_norm"] = bool(cfg["track_grad_norm"])
    fit_kw = {"epochs": int(cfg["epochs"]), "batch_size": int(cfg["batch_size"]), "lr0": float(cfg["lr"]), "eta_min": float(cfg["eta_min"]),
              "log_every": int(cfg["log_every"]), "test_every": int(cfg["test_every"]), "cutmix": bool(cfg.get("cutmix", False)),
              "cutout": bool(cfg.get("cutout", False)), "patch_size": int(cfg["patch_size"]), "save_image": bool(cfg.get("save_image", False)),
              "preview_every": int(cfg.get("preview_every", 200)), "validate_ema": bool(cfg.get("validate_ema", False)),
              "seed": int(cfg.get("seed", 33)), "ring_rows": int(cfg.get("ring_rows", 1024))}
    dataset = str(cfg.get("training_dataset", "us1k"))
    if dataset not in ("us1k", "folder"):
        raise M2TError(f"training_dataset must be 'us1k' or 'folder', got {dataset!r}")
    if dataset == "folder" and not cfg.get("train_hr_path"):
        raise M2TError("training_dataset: folder needs train_hr_path")
    if dataset == "us1k" and not cfg.get("data_path"):
        raise M2TError("training_dataset: us1k needs data_path")
    eval_sets = list(cfg.get("eval_sets") or [])
    bad = [n for n in eval_sets if n not in EVAL_SETS]
    if bad:
        raise M2TError(f"eval_sets knows {sorted(EVAL_SETS)}, got {bad} (any other folder goes under eval_folders)")
    data = {"training_dataset": dataset, "data_path": cfg.get("data_path"), "train_hr_path": cfg.get("train_hr_path"),
            "eval_sets": eval_sets, "eval_folders": dict(cfg.get("eval_folders") or {}), "scale": int(cfg["scale"]),
            "colors": int(model["colors"]), "patch_size": int(cfg["patch_size"]), "data_repeat": int(cfg.get("data_repeat", 1)),
            "data_augment": bool(cfg.get("data_augment", True))}
    if degradation is not None:
        data["degradation"] = degradation
    return {"model": model, "train_step": ts, "fit": fit_kw, "data": data, "pretrain": cfg.get("pretrain"),
            "log_path": str(cfg.get("log_path") or "./experiments"), "log_name": cfg.get("log_name"),
            "ignored": [k for k in IGNORED_KEYS if k in cfg]}


def timestamp_str(now=None) -> str:
    """utils.cur_timestamp_str: YYYY-MMDD-HHMM."""
    now = now or datetime.datetime.now()
    return "{}-{}{}-{}{}".format(now.year, str(now.month).zfill(2), str(now.day).zfill(2), str(now.hour).zfill(2), str(now.minute).zfill(2))


def experiment_dir(log_path: str, log_name, model: str, scale: int, stamp: str) -> str:
    """train.py:110-117: `<log_path>/<model>-fp32-x<scale>-<stamp>`, or `<log_path>/<log_name>-<stamp>` (the reference writes
    'fp32' into the name whatever the run computes in; kept)."""
    name = "{}-{}-x{}-{}".format(model, "fp32", scale, stamp) if log_name is None else "{}-{}".format(log_name, stamp)
    return os.path.join(log_path, name)


def build_datasets(data: dict, device="cuda"):
    """(US1K, [(name, Benchmark)]) in the folder layout of datas/utils.py:7-53, or from plain folders."""
    from .datas import US1K, Benchmark
    from .degrade import from_config
    from .infer import image_names
    degradation = from_config(data["scale"], data.get("degradation"))
    common = dict(train=True, augment=data["data_augment"], scale=data["scale"], colors=data["colors"], patch_size=data["patch_size"],
                  repeat=data["data_repeat"], device=device)
    if data["training_dataset"] == "folder":
        from PIL import Image
        folder = str(data["train_hr_path"])
        images = [(np.asarray(Image.open(os.path.join(folder, n)).convert("RGB")), None) for n in image_names(folder)]
        if not images:
            raise M2TError(f"train_hr_path {folder}: no image file")
        train = US1K(images=images, degradation=degradation, **common)
    else:
        root = str(data["data_path"])
        train = US1K(os.path.join(root, "US1K/US1K_train_HR"), None if degradation is not None else os.path.join(root, "US1K/US1K_train_LR_bicubic"),
                     os.path.join(root, "us1k_cache"), degradation=degradation, **common)
    valid = []
    for name in data["eval_sets"]:
        base = os.path.join(str(data["data_path"]), "benchmark", EVAL_SETS[name])
        valid.append((name, Benchmark(os.path.join(base, "HR"), os.path.join(base, "LR_bicubic"), scale=data["scale"],
                                      colors=data["colors"], device=device)))
    for name, hr_dir in data["eval_folders"].items():
        valid.append((str(name), Benchmark(str(hr_dir), None, scale=data["scale"], colors=data["colors"], device=device,
                                           degradation=degradation)))
    return train, valid


class _Tee:
    """utils.ExperimentLogger: stdout and log.txt."""

    def __init__(self, filename, stream):
        self.terminal, self.log = stream, open(filename, "a")

    def write(self, message):
        self.terminal.write(message)
        self.log.write(message)

    def flush(self):
        self.terminal.flush()
        self.log.flush()


def main(argv=None) -> int:
    args = parse_args(argv)
    import yaml
    from .infer import load_weights, model_namespace
    from .M2Trans_network import create_model
    from .train_step import TrainStep
    with open(args.config) as f:
        cfg = yaml.load(f, Loader=yaml.FullLoader) or {}
    cfg = apply_overrides(cfg, args.set)
    r = resolve_config(cfg, args.compute_dtype)
    if not torch.cuda.is_available():
        raise M2TError("python -m m2trans_amd.train needs a HIP device: there is no host fallback")
    if args.resume is not None:
        out_dir = args.resume
        os.makedirs(out_dir, exist_ok=True)
    else:
        out_dir = experiment_dir(r["log_path"], r["log_name"], "M2Trans", r["data"]["scale"], timestamp_str())
        os.makedirs(out_dir, exist_ok=True)
        _dump_yaml(dict(cfg, config=args.config, resume=args.resume), os.path.join(out_dir, "config.yml"))
    stdout = sys.stdout
    sys.stdout = _Tee(os.path.join(out_dir, "log.txt"), stdout)
    try:
        if r["ignored"]:
            print(f"## accepted and ignored: {', '.join(r['ignored'])} (one device, no loader workers, the head count is fixed) ##")
        model = create_model(model_namespace(r["model"])).to("cuda")
        if r["pretrain"]:
            print("## load pretrained model: {}! ##".format(r["pretrain"]))
            load_weights(model, torch.load(r["pretrain"], map_location="cpu", weights_only=False))
        print(model)
        ts = TrainStep(model, **r["train_step"])
        train, valid = build_datasets(r["data"])
        print("##=== select {} for evaluation! ===##".format(" ".join(n for n, _ in valid)) if valid else "select no dataset for evaluation!")
        fit(model, ts, train, valid, out_dir=out_dir, resume=args.resume, **r["fit"])
    finally:
        sys.stdout.flush()
        sys.stdout = stdout
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
