"""Checkpoint wire format of the reference (train.py:341-349 save, :85-108 resume, test.py:64-70 load).

    torch.save({'epoch', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict', 'stat_dict'}, path)

* model keys carry DataParallel's ``module.`` prefix (train.py:73);
* optimizer_state_dict is torch.optim.Adam's: per-parameter ``step``/``exp_avg``/``exp_avg_sq`` indexed in
  ``model.parameters()`` order with the 4 frozen MeanShift tensors included (the reference passes every
  parameter to Adam, train.py:81; frozen ones simply never get state);
* scheduler_state_dict is CosineAnnealingLR's.  The reference saves inside the epoch loop BEFORE ``scheduler.step()``
  (train.py:341-358), so the checkpoint of epoch E (1-based) holds ``last_epoch = E - 1``, ``_step_count = E`` and the
  learning rate epoch E trained with, cosine(E - 1).

Both dicts are produced by REAL ``torch.optim.Adam`` / ``CosineAnnealingLR`` objects built the way train.py:81-82
builds them (so every key the installed torch writes is present with torch's own value), then filled with the
fused step driver's flat moment buffers.  Pinned: the reference's model, optimiser and scheduler run through two
epochs and saved as train.py:341-349 does give the committed manifest ``tests/golden/checkpoint_manifest.json``
(written by the pinning script of the test infrastructure); ``tests/test_host_cpu.py`` requires ``export_checkpoint``
to match it key for key.

With TrainStep's optimizer options on (max_grad_norm, weight_decay, ema_decay, skip_nonfinite) the dict additionally carries:
the decay in torch's own ``param_groups`` (``weight_decay``, ``decoupled_weight_decay``), the APPLIED step number in every
``step`` (optimizer steps that skip_nonfinite left out never happened), ``ema_state_dict`` (``module.``-prefixed, loadable
strictly) and ``m2t_optim`` = {max_grad_norm, ema_decay, skip_nonfinite, skipped_steps}.  With every option off it is the dict
above, key for key.

With a pixel loss other than L1 (TrainStep(pixel_loss=...)) the dict carries ``m2t_loss`` = {"pixel_loss": name, "param": eps /
beta / None}; ``import_checkpoint`` sets the TrainStep's loss from it and leaves the loss alone when the file has no such entry.
An L1 run writes no entry: its dict is the one above.  Every optional loss term of the step that is on (the rows of
train_step.LOSS_TERMS and the perceptual term, in the order of LOSS_KEY_ORDER below, which is not the call order) adds its weight to
the entry as ``"lambda_<term>"`` (and the entry then exists for an L1 pixel term too); ``import_checkpoint`` calls the step's
``set_lambda_<term>`` with it.  ``"lambda_fft"`` is followed by ``"fft_norm"``; ``"lambda_wavelet"`` by ``"wavelet"`` (a name or the two
tap lists), ``"wavelet_levels"``, ``"wavelet_band_weights"`` and ``"wavelet_eps"``; ``"lambda_consistency"`` by ``"consistency_eps"``;
``"lambda_perceptual"`` by ``"perceptual_criterion"``, ``"perceptual_weights"`` and ``"perceptual_resize"`` (never the VGG19 weights;
``import_checkpoint`` sets them on the step's ``perceptual_loss`` object first).  The keys of a term whose weight is 0 are absent, so
with every weight 0 the dict is the one described above, byte for byte.

With TrainStep(param_groups=...) the optimizer dict comes from a real ``torch.optim.Adam`` with ONE TORCH PARAM GROUP PER GROUP, each
carrying its own ``lr`` (= step.lr * lr_scale) and ``weight_decay``; the parameter ids run through the groups in order (torch's own
numbering), the 4 frozen MeanShift tensors at the end of the last group.  Frozen tensors are listed in their group's ``params`` and
have no ``state`` entry, like a torch Adam that never saw their gradient; ``import_checkpoint`` reads a missing entry as zero
moments.  The dict gains ``m2t_groups`` = {"spec": the spec as given, "groups": the resolved groups (tensor names, lr_scale,
weight_decay or None = the step's, frozen), "lr", "weight_decay", "decoupled_weight_decay": the step's own values}.
``import_checkpoint`` requires the step it loads into to have been built with the same groups: a mismatch is an M2TError that names
the difference.  Without groups the dict is the one above, key for key.
"""
from __future__ import annotations

import warnings
from typing import Dict, Optional

import torch


def _param_index(model) -> Dict[str, int]:
    return {n: i for i, (n, _) in enumerate(model.named_parameters())}


def ema_state_dict(model, ema_params) -> dict:
    """The flat EMA buffer under the model's own state_dict names, as copies; the frozen MeanShift entries (and anything else
    outside the flat buffer) are the model's, so ``model.load_state_dict(..., strict=True)`` accepts it."""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for n, (o, k, shp) in zip(model._names, model._slots):
        sd[n] = ema_params[o:o + k].view(shp).detach().clone()
    return sd


def _groups(train_step):
    return getattr(train_step, "groups", None)


def _torch_group_names(model, groups) -> list:
    """Tensor names of each torch param group of a grouped export, in torch's id order: the groups' members, then -- at the end of
    the last group -- every parameter outside the flat buffer (the frozen MeanShift tensors)."""
    out = [list(m) for m in groups.members]
    flat = set(model._names)
    out[-1] = out[-1] + [n for n, _ in model.named_parameters() if n not in flat]
    return out


def _check_groups(ckpt: dict, train_step):
    """A grouped optimizer state loads only into a step built with the same groups (and a group-free one into a group-free step)."""
    from ._lib import M2TError
    from .param_groups import describe_difference
    mg, g = ckpt.get("m2t_groups"), _groups(train_step)
    if mg is None and g is None:
        return
    if mg is None:
        raise M2TError("import_checkpoint: the checkpoint was written without parameter groups, this TrainStep was built with "
                       f"param_groups={g.spec!r}")
    if g is None:
        raise M2TError(f"import_checkpoint: the checkpoint was written with param_groups={mg.get('spec')!r}, this TrainStep was "
                       "built without parameter groups")
    diff = describe_difference(mg["groups"], g.describe())
    if diff is not None:
        raise M2TError(f"import_checkpoint: the checkpoint's parameter groups are not this TrainStep's: {diff} (checkpoint spec "
                       f"{mg.get('spec')!r}, this step's {g.spec!r})")


def _optim_options(train_step) -> dict:
    """TrainStep's optimizer options, read with their "off" defaults (an object without them exports as before)."""
    return {"max_grad_norm": getattr(train_step, "max_grad_norm", None),
            "weight_decay": float(getattr(train_step, "weight_decay", 0.0)),
            "decoupled_weight_decay": bool(getattr(train_step, "decoupled_weight_decay", False)),
            "ema_decay": getattr(train_step, "ema_decay", None),
            "skip_nonfinite": bool(getattr(train_step, "skip_nonfinite", False))}


# the order of the "lambda_<term>" keys of the ``m2t_loss`` entry: the order in which the terms came to the file format, kept so that a
# checkpoint comes out byte for byte as it always did.  The names are those of train_step.LOSS_TERMS plus the perceptual term.
LOSS_KEY_ORDER = ("ssim", "msssim", "fft", "vif", "perceptual", "gmsd", "wavelet", "consistency")


def _pixel_loss(train_step):
    """The ``m2t_loss`` entry of a step object, or None for L1 with every optional term off (and for an object that knows no pixel
    losses)."""
    from .train_step import resolve_pixel_loss
    _, canon, value = resolve_pixel_loss(getattr(train_step, "pixel_loss", "l1"), getattr(train_step, "pixel_loss_param", None))
    lam = {n: float(getattr(train_step, f"lambda_{n}", 0.0) or 0.0) for n in LOSS_KEY_ORDER}
    if canon == "l1" and not any(lam.values()):
        return None
    out = {"pixel_loss": canon, "param": value}
    for n in LOSS_KEY_ORDER:
        if lam[n] == 0.0:
            continue
        out[f"lambda_{n}"] = lam[n]
        if n == "fft":
            out["fft_norm"] = str(getattr(train_step, "fft_norm", "backward"))
        if n == "wavelet":
            w = getattr(train_step, "wavelet", "haar")
            out["wavelet"] = w if isinstance(w, str) else [[float(v) for v in f] for f in w]
            out["wavelet_levels"] = int(getattr(train_step, "wavelet_levels", 2))
            bw = getattr(train_step, "wavelet_band_weights", None)
            out["wavelet_band_weights"] = None if bw is None else [float(v) for v in bw]
            out["wavelet_eps"] = float(getattr(train_step, "wavelet_eps", 0.0))
        if n == "consistency":
            out["consistency_eps"] = float(getattr(train_step, "consistency_eps", 0.0))
        if n == "perceptual":
            # the settings of the term, never the VGG19 weights (an integrator loads those: INTEGRATION.md)
            p = train_step.perceptual_loss
            out["perceptual_criterion"] = str(p.criterion)
            out["perceptual_weights"] = [float(w) for w in p.weights]
            out["perceptual_resize"] = bool(p.resize)
    return out


def _skipped(train_step) -> int:
    s = getattr(train_step, "skipped_steps", None)
    return 0 if s is None else int(float(s))


def _reset_optim_state(train_step, model, ema_sd=None):
    """After a load: the skipped count restarts at 0 (step_count is the applied count from here on) and the EMA weights come
    from the file, or -- when it has none -- from the weights just loaded."""
    rec = getattr(train_step, "optim_record", None)
    if rec is not None:
        rec.zero_()
    ema = getattr(train_step, "ema_params", None)
    if ema is None:
        return
    with torch.no_grad():
        if ema_sd is None:
            ema.copy_(model.flat_params.detach().to(ema))
            return
        for n, (o, k, shp) in zip(model._names, model._slots):
            v = ema_sd["module." + n] if ("module." + n) in ema_sd else ema_sd[n]
            ema[o:o + k].copy_(v.reshape(-1).to(ema))


def export_checkpoint(model, train_step=None, epoch: int = 1, stat_dict: Optional[dict] = None,
                      lr0: float = 1e-4, eta_min: float = 1e-6, t_max: float = 200.0) -> dict:
    """The dict train.py:341-349 saves at the end of (1-based) epoch `epoch`."""
    if train_step is not None and getattr(train_step, "micro_count", 0) != 0:
        # TrainStep(accum_steps=k): the moments are one optimizer step behind gradients that are half summed and that no
        # checkpoint format carries
        from ._lib import M2TError
        raise M2TError(f"export_checkpoint in the middle of an accumulation cycle ({train_step.micro_count} of "
                       f"{getattr(train_step, 'accum_steps', '?')} micro-batches since the last optimizer step)")
    sd ={"module." + k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    out = {"epoch": int(epoch), "model_state_dict": sd}
    if train_step is not None:
        params = [p for _, p in model.named_parameters()]                 # ALL parameters, like train.py:81
        oo = _optim_options(train_step)
        options_on = (oo["max_grad_norm"] is not None or oo["weight_decay"] != 0.0 or oo["ema_decay"] is not None
                      or oo["skip_nonfinite"])
        groups = _groups(train_step)
        by_name = dict(model.named_parameters())
        if groups is not None:
            # one torch param group per group, with its own lr and weight decay (the schedule scales each group's lr0 alike)
            wds = groups.group_weight_decay(oo["weight_decay"])
            tg = [{"params": [by_name[n] for n in names], "lr": lr0 * groups.lr_scale[g], "weight_decay": wds[g]}
                  for g, names in enumerate(_torch_group_names(model, groups))]
            kw = {"decoupled_weight_decay": oo["decoupled_weight_decay"]} if any(w != 0.0 for w in wds) else {}
            opt = torch.optim.Adam(tg, lr=lr0, weight_decay=0, **kw)
        elif oo["weight_decay"] != 0.0:
            # torch's own param_groups carry the decay (decoupled_weight_decay is Adam's AdamW switch)
            opt = torch.optim.Adam(params, lr=lr0, weight_decay=oo["weight_decay"],
                                   decoupled_weight_decay=oo["decoupled_weight_decay"])
        else:
            opt = torch.optim.Adam(params, lr=lr0, weight_decay=0)
        skipped = _skipped(train_step)
        applied = int(train_step.step_count) - skipped                    # Adam's step number: skipped steps never happened
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, float(t_max), eta_min=eta_min)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                               # "scheduler.step() before optimizer.step()"
            for _ in range(max(0, int(epoch) - 1)):                       # epochs 1 .. E-1 have stepped the scheduler
                sched.step()
        # the learning rate the step driver really used (equals the schedule's when the caller follows cosine_lr)
        if groups is not None:
            lrs = groups.group_lr(train_step.lr)
            for pg, lr_g in zip(opt.param_groups, lrs):
                pg["lr"] = lr_g
            sched._last_lr = list(lrs)
        else:
            opt.param_groups[0]["lr"] = float(train_step.lr)
            sched._last_lr = [float(train_step.lr)]
        if applied > 0:
            idx = _param_index(model)
            frozen = set(groups.frozen_names()) if groups is not None else ()
            for n, (o, k, shp) in zip(model._names, model._slots):
                if n in frozen:
                    continue                                              # like a torch Adam that never saw this gradient
                p = params[idx[n]]
                opt.state[p] = {"step": torch.tensor(float(applied)),
                                "exp_avg": train_step.exp_avg[o:o + k].view(shp).detach().cpu().clone(),
                                "exp_avg_sq": train_step.exp_avg_sq[o:o + k].view(shp).detach().cpu().clone()}
        out["optimizer_state_dict"] = opt.state_dict()
        out["scheduler_state_dict"] = sched.state_dict()
    out["stat_dict"] = stat_dict or {}
    if train_step is not None and options_on:
        if getattr(train_step, "ema_params", None) is not None:
            out["ema_state_dict"] = {"module." + k: v.cpu() for k, v in ema_state_dict(model, train_step.ema_params).items()}
        out["m2t_optim"] = {"max_grad_norm": oo["max_grad_norm"], "ema_decay": oo["ema_decay"],
                            "skip_nonfinite": oo["skip_nonfinite"], "skipped_steps": skipped}
    if train_step is not None and _pixel_loss(train_step) is not None:
        out["m2t_loss"] = _pixel_loss(train_step)
    if train_step is not None and _groups(train_step) is not None:
        g = _groups(train_step)
        out["m2t_groups"] = {"spec": g.spec, "groups": g.describe(), "lr": float(train_step.lr),
                             "weight_decay": oo["weight_decay"], "decoupled_weight_decay": oo["decoupled_weight_decay"]}
    return out


def import_checkpoint(ckpt: dict, model, train_step=None) -> int:
    """Load a reference-format checkpoint; returns the epoch to continue from (train.py:97-100).
    The learning rate comes from the optimizer's param_groups (what `optimizer.load_state_dict` restores); the
    scheduler's position is kept in ``train_step.scheduler_last_epoch`` so the caller can continue the cosine
    schedule with ``cosine_lr(train_step.scheduler_last_epoch + k)`` after k further scheduler steps -- like the
    reference, whose resumed run re-uses the saved epoch's rate for its first epoch (train.py:103,358)."""
    model.load_state_dict(ckpt["model_state_dict"], strict=True)
    if train_step is None:
        return int(ckpt.get("epoch", 0)) + 1
    ml = ckpt.get("m2t_loss")
    if ml is not None:
        # the pixel loss the run was saved with (a file without the entry leaves the TrainStep's own untouched)
        if hasattr(train_step, "set_pixel_loss"):
            train_step.set_pixel_loss(ml["pixel_loss"], ml.get("param"))
        else:
            from .train_step import resolve_pixel_loss
            _, train_step.pixel_loss, train_step.pixel_loss_param = resolve_pixel_loss(ml["pixel_loss"], ml.get("param"))
        from .train_step import LOSS_TERMS, resolve_consistency_eps, resolve_fft_norm, resolve_lambda, resolve_wavelet
        for t in LOSS_TERMS:           # (a file without a term's key leaves that weight alone: 0 on a fresh step)
            key = f"lambda_{t.name}"
            if key not in ml:
                continue
            more = ()
            if t.name == "fft":
                more = (ml.get("fft_norm"),)
            if t.name == "wavelet":
                # (the file's own settings, whatever the importing step was built with: absent weights are the default ones)
                w = resolve_wavelet(ml.get("wavelet", "haar"), ml.get("wavelet_levels", 2), ml.get("wavelet_band_weights"),
                                    ml.get("wavelet_eps", 0.0))
                if hasattr(train_step, "wavelet_band_weights"):
                    train_step.wavelet_band_weights = None
                more = (w.wavelet, w.levels, w.band_weights, w.eps)
            if t.name == "consistency":
                more = (ml.get("consistency_eps", 0.0),)
            if hasattr(train_step, f"set_{key}"):
                getattr(train_step, f"set_{key}")(ml[key], *more)
            else:
                # a stand-in step object without the setters receives the attributes
                setattr(train_step, key, resolve_lambda(t.name, ml[key]))
                if t.name == "fft":
                    train_step.fft_norm = resolve_fft_norm(ml.get("fft_norm", "backward"))
                if t.name == "wavelet":
                    train_step.wavelet, train_step.wavelet_levels, train_step.wavelet_eps = w.wavelet, w.levels, w.eps
                    train_step.wavelet_band_weights = None if w.band_weights is None else list(w.band_weights)
                if t.name == "consistency":
                    train_step.consistency_eps = resolve_consistency_eps(more[0])
        if "lambda_perceptual" in ml:
            p = getattr(train_step, "perceptual_loss", None)
            if p is None:
                from ._lib import M2TError
                raise M2TError("import_checkpoint: the file was saved with lambda_perceptual > 0; build the TrainStep with "
                               "perceptual_loss= (a losses.PerceptualLoss with VGG19 weights loaded: the file carries none)")
            p.configure(ml.get("perceptual_weights", p.weights), ml.get("perceptual_criterion", p.criterion),
                        ml.get("perceptual_resize", p.resize))
            train_step.set_lambda_perceptual(ml["lambda_perceptual"])
    opt = ckpt.get("optimizer_state_dict") or {}
    sch = ckpt.get("scheduler_state_dict")
    if not opt.get("state") and not opt.get("param_groups") and sch is None:
        # weights only = the reference's --pretrain load (train.py:85-88): model weights alone, fresh Adam moments, fresh
        # CosineAnnealingLR, start_epoch stays 1 (train.py:62)
        train_step.exp_avg.zero_()
        train_step.exp_avg_sq.zero_()
        train_step.step_count = 0
        train_step.scheduler_last_epoch = 0
        _reset_optim_state(train_step, model, ckpt.get("ema_state_dict"))
        return 1
    _check_groups(ckpt, train_step)
    groups, mg = _groups(train_step), ckpt.get("m2t_groups")
    if sch is None:
        # Adam state without the schedule it belongs to: the reference's --resume (train.py:97-103) always loads both, and
        # continuing epoch-N moments / learning rate on a schedule restarted at 0 would silently train something else
        raise ValueError("checkpoint carries optimizer_state_dict but no scheduler_state_dict: not a resume checkpoint of "
                         "train.py:341-349; pass the model weights alone (a --pretrain load) or a complete checkpoint")
    if opt.get("state"):
        idx = _param_index(model)
        if groups is not None:                                            # torch numbers the parameters through the groups in order
            idx = {n: i for i, n in enumerate(n for names in _torch_group_names(model, groups) for n in names)}
        st = opt["state"]
        step = 0
        for n, (o, k, shp) in zip(model._names, model._slots):
            s = st.get(idx[n]) or st.get(str(idx[n]))
            if s is None:
                if groups is not None:                                    # no state entry = zero moments (a frozen tensor)
                    train_step.exp_avg[o:o + k].zero_()
                    train_step.exp_avg_sq[o:o + k].zero_()
                continue
            train_step.exp_avg[o:o + k].copy_(s["exp_avg"].reshape(-1).to(train_step.exp_avg))
            train_step.exp_avg_sq[o:o + k].copy_(s["exp_avg_sq"].reshape(-1).to(train_step.exp_avg_sq))
            step = int(float(s["step"]))
        train_step.step_count = step
    else:
        # a resume checkpoint written before the first optimizer step: optimizer.load_state_dict (train.py:101) would leave an EMPTY
        # Adam state, i.e. zero moments and step 0 -- not whatever this TrainStep accumulated before the load
        train_step.exp_avg.zero_()
        train_step.exp_avg_sq.zero_()
        train_step.step_count = 0
    pg = opt.get("param_groups")
    if mg is not None:
        train_step.set_lr(mg["lr"])                                       # the step's own rate: each group's is lr * lr_scale
    elif pg:
        train_step.set_lr(pg[0]["lr"])
    mo = ckpt.get("m2t_optim")
    wd = float(pg[0].get("weight_decay", 0.0) or 0.0) if pg else 0.0
    if mg is not None:                                                    # (torch's groups carry each group's decay; the step's own:)
        wd = float(mg["weight_decay"])
    if mo is not None or wd != 0.0:
        # the options the run was saved with (a file without them leaves the TrainStep's own untouched)
        mo = mo or {}
        new = {"max_grad_norm": mo.get("max_grad_norm", getattr(train_step, "max_grad_norm", None)), "weight_decay": wd,
               "decoupled_weight_decay": bool(mg["decoupled_weight_decay"]) if mg is not None else
                                         bool(pg[0].get("decoupled_weight_decay", False)) if pg else False,
               "ema_decay": mo.get("ema_decay", getattr(train_step, "ema_decay", None)),
               "skip_nonfinite": bool(mo.get("skip_nonfinite", getattr(train_step, "skip_nonfinite", False)))}
        if new != _optim_options(train_step):
            if hasattr(train_step, "_init_optim_options"):       # TrainStep: (re)allocates the record and the EMA buffer it needs
                train_step._init_optim_options(track_grad_norm=getattr(train_step, "track_grad_norm", False), **new)
            else:
                for k, v in new.items():
                    setattr(train_step, k, v)
    _reset_optim_state(train_step, model, ckpt.get("ema_state_dict"))
    train_step.scheduler_last_epoch = int(sch.get("last_epoch", 0))
    return int(ckpt.get("epoch", 0)) + 1
