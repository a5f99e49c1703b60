"""Helpers shared by the -m gpu parity tests (HIP path vs the CPU oracle)."""
from __future__ import annotations

import types

import torch

from oracle import m2trans_oracle as O


def make_args(scale=4, n_blocks=8, compute_dtype="fp32"):
    return types.SimpleNamespace(n_feats=64, scale=scale, rgb_range=1.0, n_blocks=n_blocks, colors=3,
                                 compute_dtype=compute_dtype)


def build_model(scale, n_blocks, compute_dtype="fp32", params=None, device="cuda"):
    from m2trans_amd.M2Trans_network import create_model
    model = create_model(make_args(scale, n_blocks, compute_dtype))
    if params is None:
        params = O.closed_form_params(64, scale, n_blocks)
    torch.nn.Module.load_state_dict(model, {k: v.clone() for k, v in params.items()}, strict=True)
    return model.to(device), params


def nchw_to_nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2).contiguous()


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def rms_rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def ws_nchw(plan, name, B, H, W, C):
    """Workspace tensor (NHWC in the plan's dtype) -> float32 NCHW on the CPU.  The 64-channel low-resolution
    feature maps (X_b, b*.xc) are chunk-planar ("P64": [4][B*H*W][16], csrc/m2t_common.h)."""
    import re
    t = plan.ws_tensor(name)
    if C == 64 and re.fullmatch(r"X\d+|b\d+\.xc", name):
        t = t.view(4, B, H, W, 16).permute(1, 2, 3, 0, 4).reshape(B, H, W, 64)
        return nhwc_to_nchw(t.float()).cpu()
    return nhwc_to_nchw(t.view(B, H, W, C).float()).cpu()


BR_C = (16, 64, 256, 256)
BR_L = (0, 1, 2, 2)


# ------------------------------------------------------------------ schedule / stale-read gates (tests/test_gpu_schedule.py)
def set_options(model, x, **opts):
    """m2t_set_option on the plan of x's shape (created if need be); returns the plan."""
    from m2trans_amd import _lib
    plan = model._plan_for(x)
    for k, v in opts.items():
        _lib.check(_lib.load().m2t_set_option(plan.handle, k.encode(), int(v)), "m2t_set_option " + k)
    return plan


def differing_tensors(model, a: torch.Tensor, b: torch.Tensor):
    """Names of the parameter tensors in whose range two flat buffers (gradients, parameters, Adam moments) differ."""
    return [n for n, (o, k) in model.param_offsets().items() if not torch.equal(a[o:o + k], b[o:o + k])]


def assert_flat_equal(model, a: torch.Tensor, b: torch.Tensor, what: str):
    """torch.equal on two flat buffers; the failure names the differing parameter tensors (they place a missing stream edge:
    a stage's weight gradients are produced by that stage's side-stream launches)."""
    if not torch.equal(a, b):
        bad = differing_tensors(model, a, b)
        raise AssertionError(f"{what}: differ in {bad[:8]} ({len(bad)} of {len(model.param_offsets())} tensors)")


# workspace regions that carry indices or descriptors, or that must hold zeros: never poisoned by name.  pack_descs, pack_blocks and
# zero_page are (re)written by m2t_plan_init_workspace, red_descs by the first backward pass after it (include/m2t.h)
WS_PERSISTENT = ("zero_page", "pack_descs", "pack_blocks", "red_descs")


def ws_float_regions(plan):
    """[(name, byte offset, bytes)] of every floating-point region of the plan's workspace, by the names m2t_plan_create registers.
    Fails if these regions and WS_PERSISTENT together do not tile workspace_bytes exactly (up to the 256-byte alignment of each
    region): a region added to the library later cannot silently escape the poison of the history-independence tests."""
    nb, s = plan.n_blocks, plan.scale
    from m2trans_amd import _lib
    T, F = (4 if plan.dtype == _lib.F32 else 2), 4      # element size of a region: the plan's compute type, or always fp32
    names = [("packed", T)] + [(f"X{b}", T) for b in range(nb + 1)]
    for b in range(nb):
        names += [(f"b{b}.mean", F), (f"b{b}.rstd", F), (f"b{b}.xc", T)]
        for i in range(1, 5):
            names += [(f"b{b}.d{i}", T), (f"b{b}.qkv{i}", T)]
    names += [("xin", T), ("a", T), ("norm_part", F), ("norm_s", F), ("vring", T), ("norm_part0", F), ("t1act", T), ("t1der", T)]
    if s == 4:
        names += [("t2act", T), ("t2der", T)]
    names += [("srpre", F), ("loss_part", F), ("gpre", F)]
    if s == 4:
        names += [("g_t2pre", T)]
    names += [("g_t1pre", T)] + [(n, T) for n in ("gT", "gA", "gB", "gxc", "gn", "ga", "gd", "gd2", "gdwin2", "gdwin", "head_cols")]
    for i in range(4):
        for sfx in ("", "b"):
            names += [(f"gqkv{i}{sfx}", T), (f"win{i}{sfx}", T), (f"relw{i}{sfx}", F)]
    names += [("rel_part", F), ("arena", F), ("col_part", F)]
    regions = [(n, plan.query("ws:" + n), plan.query("wsn:" + n) * e) for n, e in names]
    every = regions + [(n, plan.query("ws:" + n), plan.query("wsn:" + n)) for n in WS_PERSISTENT]      # (byte-sized regions)
    end = 0
    for n, off, nbytes in sorted(every, key=lambda r: (r[1], r[2])):
        if off != (end + 255) // 256 * 256:
            raise AssertionError(f"workspace region list out of date: {n} starts at byte {off}, the listed regions before it end at {end}")
        end = off + nbytes
    total = plan.query("workspace_bytes")
    if (end + 255) // 256 * 256 != total:
        raise AssertionError(f"workspace region list out of date: the listed regions end at byte {end} of {total}")
    return regions


def poison_float_regions(plan):
    """0xFF (NaN as bf16 and as fp32) into every floating-point workspace region, by name."""
    for _, off, nbytes in ws_float_regions(plan):
        plan.workspace[off:off + nbytes].fill_(0xFF)


def poison_whole_workspace(plan):
    """0xFF into the WHOLE workspace, then m2t_plan_init_workspace again: legal on a live plan, which is then back to
    'no activations, no seed, reduction table not published' (include/m2t.h)."""
    from m2trans_amd import _lib
    ws_float_regions(plan)                      # (the inventory check: no unknown index-carrying region is about to be poisoned)
    plan.workspace.fill_(0xFF)
    _lib.check(_lib.load().m2t_plan_init_workspace(plan.handle, _lib.ptr(plan.workspace), _lib.stream_ptr()),
               "m2t_plan_init_workspace")


def hip_forward_trace(plan, scale, n_blocks, B, H, W):
    """Every stored activation of the last m2t_forward, read back from the workspace as float32 NCHW on the CPU, under the
    names the oracle's ``force`` / ``cap`` dicts use (H, W = padded LR size)."""
    t = {"X0": ws_nchw(plan, "X0", B, H, W, 64)}
    for b in range(n_blocks):
        for nm in ("mean", "rstd"):                        # InstanceNorm statistics of the block input: [B, 64], fp32 in both compute types
            t[f"b{b}.{nm}"] = plan.ws_tensor(f"b{b}.{nm}", dtype=torch.float32).view(B, 64).cpu().clone()
        for i in range(4):
            h, w = H >> BR_L[i], W >> BR_L[i]
            t[f"b{b}.d{i+1}"] = ws_nchw(plan, f"b{b}.d{i+1}", B, h, w, BR_C[i])
            if i > 1 or plan.query(f"stores_qkv{i+1}") == 1:   # (bf16 default: q | k | v of the C = 16 / 64 branches are recomputed by the backward)
                t[f"b{b}.qkv{i+1}"] = ws_nchw(plan, f"b{b}.qkv{i+1}", B, h, w, 3 * BR_C[i])
        t[f"b{b}.xc"] = ws_nchw(plan, f"b{b}.xc", B, H, W, 64)
        t[f"X{b+1}"] = ws_nchw(plan, f"X{b+1}", B, H, W, 64)
    r0 = 2 if scale == 4 else scale
    if plan.query("stores_t1") == 1:                       # (x2 / x3 bf16: the row-streaming tail keeps gelu(t) / gelu'(t) in registers)
        for nm in ("t1act", "t1der"):
            t[nm] = ws_nchw(plan, nm, B, H * r0, W * r0, 64)
    if scale == 4 and plan.query("stores_t2") == 1:        # the fused forward tail keeps gelu(t2) / gelu'(t2) in LDS
        for nm in ("t2act", "t2der"):
            t[nm] = ws_nchw(plan, nm, B, H * 4, W * 4, 64)
    t["srpre"] = plan.ws_tensor("srpre", dtype=torch.float32).view(B, 3, H * scale, W * scale).cpu().clone()
    return t


def _ws_p64(plan, name, B, H, W):
    """A chunk-planar 64-channel workspace tensor ([4][B*H*W][16], csrc/m2t_common.h) -> float32 NCHW on the CPU."""
    t = plan.ws_tensor(name).view(4, B, H, W, 16).permute(1, 2, 3, 0, 4).reshape(B, H, W, 64)
    return nhwc_to_nchw(t.float()).cpu()


def hip_backward_trace(plan, scale, n_blocks, B, H, W):
    """The gradient tensors that the last (synchronised) m2t_backward / m2t_backward_ex left intact in the workspace, as float32 NCHW
    on the CPU under the tap names of tests/bwd_stage_ref.py (H, W = padded LR size).  Only taps that no later launch of the same pass
    overwrites are returned -- which ones those are, and which line overwrites the others, is listed in that module's docstring; they
    hold for n_blocks <= 2 (a third block would reuse buffer set 0 and gA / gB).  The input gradient is the caller's (lr.grad)."""
    if n_blocks not in (1, 2):
        raise ValueError("hip_backward_trace: the taps are intact for n_blocks <= 2 only")
    t = {"gpre": plan.ws_tensor("gpre", dtype=torch.float32).view(B, 3, H * scale, W * scale).cpu().clone()}
    if scale == 4:
        t["g_t1pre"] = nhwc_to_nchw(plan.ws_tensor("g_t1pre").view(B, 2 * H, 2 * W, 64).float()).cpu()
    t["gT"] = _ws_p64(plan, "gT", B, H, W)
    if n_blocks == 2:
        t["gB"] = _ws_p64(plan, "gB", B, H, W)
    for b in range(n_blocks):
        sfx = "b" if b & 1 else ""                         # buffer set b & 1 (csrc/m2t_api.hip: hd.gqkv[b & 1])
        for i in range(4):
            h, w = H >> BR_L[i], W >> BR_L[i]
            t[f"b{b}.gqkv{i+1}"] = nhwc_to_nchw(plan.ws_tensor(f"gqkv{i}{sfx}").view(B, h, w, 3 * BR_C[i]).float()).cpu()
    t["gn"] = _ws_p64(plan, "gn", B, H, W)                  # block 0's (the last one written)
    t["gres"] = _ws_p64(plan, "gxc", B, H, W)               # after block 0's InstanceNorm backward: g(res), the head's cotangent
    return t


def smooth_hr(B, size, seed, device="cpu", noise=0.026):
    """Band-limited synthetic 'tissue' in [0,1] (the bf16 quality tests): a low-frequency Fourier field, a few soft-edged
    blobs and mild speckle that the x4 box down-sampling removes only partly -- an image family on which the network
    reaches >= 25 dB within a few hundred steps, so that PSNR differences mean something."""
    import torch.nn.functional as F
    g = torch.Generator(device="cpu").manual_seed(seed)
    yy = torch.linspace(0, 1, size).view(1, 1, size, 1)
    xx = torch.linspace(0, 1, size).view(1, 1, 1, size)
    img = torch.zeros(B, 1, size, size)
    for _ in range(12):
        fx, fy = (torch.rand(B, 1, 1, 1, generator=g) * 14 - 7), (torch.rand(B, 1, 1, 1, generator=g) * 14 - 7)
        ph = torch.rand(B, 1, 1, 1, generator=g) * 6.283
        amp = torch.rand(B, 1, 1, 1, generator=g) * 0.12
        img = img + amp * torch.sin(6.283 * (fx * xx + fy * yy) + ph)
    for _ in range(5):
        cx, cy = torch.rand(B, 1, 1, 1, generator=g), torch.rand(B, 1, 1, 1, generator=g)
        r = 0.05 + 0.2 * torch.rand(B, 1, 1, 1, generator=g)
        a = (torch.rand(B, 1, 1, 1, generator=g) - 0.5) * 0.6
        d = ((xx - cx) ** 2 + (yy - cy) ** 2).sqrt()
        img = img + a * torch.sigmoid((r - d) * 60.0)
    speck = torch.randn(B, 1, size // 2, size // 2, generator=g)
    speck = F.interpolate(speck, size=(size, size), mode="bilinear", align_corners=False) * 0.03
    # full-resolution white speckle: the x4 box filter leaves a quarter of its amplitude in the LR image, the rest is
    # unrecoverable detail -- it caps the reachable PSNR-Y near 33 dB, the published CCA-US x4 operating point (32.72 dB)
    img = (0.45 + img + speck + noise * torch.randn(B, 1, size, size, generator=g)).clamp(0, 1)
    tint = torch.tensor([1.0, 0.97, 0.94]).view(1, 3, 1, 1)
    return (img * tint).clamp(0, 1).to(device)


def smooth_pair(B, lr_size, scale, seed, device="cpu"):
    """(LR, HR) with LR = avg_pool(HR, scale)."""
    import torch.nn.functional as F
    hr = smooth_hr(B, lr_size * scale, seed, device)
    return F.avg_pool2d(hr, scale).contiguous(), hr
