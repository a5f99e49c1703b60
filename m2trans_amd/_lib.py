"""ctypes binding of libm2t.so: ``ABI`` below is the one table of its C entry points, keyed by the public header of include/ that
declares them.

The product path has NO fallback: if the HIP library is missing, or a call fails, this
module raises.  Build it with ``python -m m2trans_amd.build`` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libm2t.so")

F32, BF16 = 0, 1

_vp, _i, _f, _d, _ll, _ull = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong, C.c_ulonglong
_dp = C.POINTER(_d)         # a HOST double array (a ctypes array, or None where the header allows NULL)

# header of include/ -> name -> (restype, argtypes): every symbol the header declares, in the header's order.  load() binds them all;
# tests/test_abi_surface_cpu.py holds each entry against its prototype type by type.
ABI = {
    "m2t.h": {
        "m2t_version": (_i, []),
        "m2t_last_error_string": (C.c_char_p, []),
        "m2t_plan_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _i]),
        "m2t_plan_destroy": (None, [_vp]),
        "m2t_plan_query": (_ll, [_vp, C.c_char_p]),
        "m2t_set_option": (_i, [_vp, C.c_char_p, _ll]),
        "m2t_stream_wait_bucket": (_i, [_vp, _i, _vp]),
        "m2t_plan_init_workspace": (_i, [_vp, _vp, _vp]),
        "m2t_forward": (_i, [_vp, _vp, _vp, _vp, _f, _i, _vp, _vp]),
        "m2t_l1_loss": (_i, [_vp, _vp, _f, _d, _f, _vp, _vp, _vp]),
        "m2t_l1_loss_deferred": (_i, [_vp, _vp, _f, _d, _f, _vp, _vp, _vp]),
        "m2t_pixel_loss": (_i, [_vp, _i, _f, _vp, _f, _d, _f, _vp, _vp, _vp]),
        "m2t_pixel_loss_deferred": (_i, [_vp, _i, _f, _vp, _f, _d, _f, _vp, _vp, _vp]),
        "m2t_set_output_grad": (_i, [_vp, _vp, _f, _vp, _vp]),
        "m2t_add_output_grad": (_i, [_vp, _vp, _i, _i, C.POINTER(_i), _f, _f, _vp, _vp]),
        "m2t_ssim_loss_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i]),
        "m2t_ssim_loss_tensor": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _i, _f, _i, _d, _vp, _vp, _i, _vp, _vp]),
        "m2t_ssim_loss": (_i, [_vp, _vp, _f, _d, _f, _vp, _i, _vp, _vp, _vp]),
        "m2t_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
        "m2t_backward_ex": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_ubyte), _vp, _vp]),
        "m2t_adam_step": (_i, [_vp, _vp, _vp, _vp, _ll, _f, _f, _f, _f, _i, _f, _vp]),
        "m2t_grad_accumulate": (_i, [_vp, _vp, _ll, _vp, _vp, _vp]),
        "m2t_grad_norm": (_i, [_vp, _ll, _f, _f, _i, _i, _f, _f, _vp, _vp, _vp]),
        "m2t_grad_norm_workspace_bytes": (_ll, []),
        "m2t_adam_step_ex": (_i, [_vp, _vp, _vp, _vp, _ll, _f, _f, _f, _f, _i, _f, _vp, _f, _i, _f, _vp, _vp]),
        "m2t_profile_enable": (_i, [_ull]),
        "m2t_profile_read": (_i, [_i, C.POINTER(_d), C.POINTER(_ll)]),
        "m2t_profile_sample_every": (_i, [_i]),
        "m2t_dwt": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
        "m2t_iwt": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
        "m2t_pixel_shuffle": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
        "m2t_pixel_unshuffle": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
        "m2t_to_nhwc": (_i, [_i, _vp, _vp, _i, _i, _i, _vp]),
        "m2t_to_nchw": (_i, [_i, _vp, _vp, _i, _i, _i, _vp]),
        "m2t_window_attention_fwd": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
        "m2t_window_attention_bwd_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
        "m2t_window_attention_bwd": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
        "m2t_swin_create": (_i, [C.POINTER(_vp), _i, _i]),
        "m2t_swin_destroy": (None, [_vp]),
        "m2t_swin_query": (_ll, [_vp, C.c_char_p]),
        "m2t_swin_param_name": (C.c_char_p, [_vp, _i]),
        "m2t_swin_load_weights": (_i, [_vp, _vp, _vp, _vp]),
        "m2t_swin_encode": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(_i), _i, _vp, _vp, _vp]),
        "m2t_swin_encode_pair": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, C.POINTER(_i), _i, _vp, _vp, _vp]),
        "m2t_semantic_loss": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
        "m2t_bicubic_resize": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
        "m2t_swin_grad_workspace_bytes": (_ll, [_vp, _i]),
        "m2t_swin_encode_grad": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, C.POINTER(_i), _i, _i, _vp, _vp, _vp, _vp]),
        "m2t_semantic_loss_backward": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
        "m2t_swin_backward": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
        "m2t_bicubic_resize_backward": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
        "m2t_text_create": (_i, [C.POINTER(_vp), _i, _i, _i]),
        "m2t_text_destroy": (None, [_vp]),
        "m2t_text_query": (_ll, [_vp, C.c_char_p]),
        "m2t_text_param_name": (C.c_char_p, [_vp, _i]),
        "m2t_text_load_weights": (_i, [_vp, _vp, _vp, _vp]),
        "m2t_text_encode": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), _i, _i, _vp, _vp, _vp]),
        "m2t_transblock_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
        "m2t_transblock_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
        "m2t_eval_metrics_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i]),
        "m2t_eval_metrics": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
        "m2t_eval_gmsd_scratch_bytes": (C.c_size_t, [_i]),
        "m2t_eval_gmsd": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
        "m2t_eval_fsim_scratch_bytes": (C.c_size_t, [_i, _i]),
        "m2t_eval_fsim": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
        "m2t_crop_patches": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
        "m2t_image_to_tensor": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
        "m2t_box_mix": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    },
    "m2t_spectral.h": {
        "m2t_fft_loss_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i]),
        "m2t_rfft2": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
        "m2t_fft_loss_tensor": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _i, _f, _i, _i, _d, _vp, _vp, _i, _vp, _vp]),
        "m2t_fft_loss": (_i, [_vp, _vp, _f, _d, _f, _i, _vp, _i, _vp, _vp, _vp]),
    },
    "m2t_resize.h": {
        "m2t_imresize_u8": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _vp]),
        "m2t_imresize_f32": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _f, _vp]),
    },
    "m2t_msssim.h": {
        "m2t_msssim_loss_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i]),
        "m2t_msssim_loss_scratch_offset": (C.c_size_t, [_i, _i, _i, _i, _i, _i]),
        "m2t_msssim_loss_tensor": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _i, _f, _i, _d, _vp, _vp, _vp, _i, _vp, _vp]),
        "m2t_msssim_loss": (_i, [_vp, _vp, _f, _d, _f, _vp, _i, _vp, _vp, _vp]),
    },
    "m2t_vif.h": {
        "m2t_vif_loss_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i]),
        "m2t_vif_loss_scratch_offset": (C.c_size_t, [_i, _i, _i, _i, _i, _i]),
        "m2t_vif_loss_tensor": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _i, _f, _d, _i, _d, _vp, _vp, _vp, _i, _vp, _vp]),
        "m2t_vif_loss": (_i, [_vp, _vp, _f, _d, _f, _d, _vp, _i, _vp, _vp, _vp]),
    },
    "m2t_groups.h": {
        "m2t_group_table_bytes": (C.c_size_t, [_i]),
        "m2t_group_table_pack": (_i, [C.POINTER(_ll), C.POINTER(_i), _i, _ll, _i, _vp]),
        "m2t_adam_step_groups": (_i, [_vp, _vp, _vp, _vp, _ll, C.POINTER(_f), _f, _f, _f, _i, _f, _vp, C.POINTER(_f), _i, _f, _vp,
                                      C.POINTER(C.c_ubyte), _i, _vp, _i, _vp]),
        "m2t_grad_norm_groups": (_i, [_vp, _ll, _f, _f, _i, _i, _f, _f, _vp, _vp, C.POINTER(C.c_ubyte), _i, _vp, _i, _vp]),
    },
    "m2t_perceptual.h": {
        "m2t_vgg_create": (_i, [C.POINTER(_vp), _i]),
        "m2t_vgg_destroy": (None, [_vp]),
        "m2t_vgg_query": (_ll, [_vp, C.c_char_p]),
        "m2t_vgg_param_name": (C.c_char_p, [_vp, _i]),
        "m2t_vgg_load_weights": (_i, [_vp, _vp, _vp, _vp]),
        "m2t_vgg_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i]),
        "m2t_vgg_workspace_offset": (C.c_size_t, [_i, _i, _i, _i, _i]),
        "m2t_vgg_loss_tensor": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _ll, _i, _f, _i, _i, _f, C.POINTER(_d), _d, _vp, _vp, _vp, _i, _vp, _vp]),
        "m2t_vgg_loss": (_i, [_vp, _vp, _vp, _f, _d, _f, _i, _f, C.POINTER(_d), _vp, _i, _vp, _vp, _vp]),
        "m2t_vgg_conv_forward": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _f, _vp]),
        "m2t_vgg_conv_backward": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
        "m2t_vgg_pool_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
        "m2t_vgg_pool_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    },
    "m2t_rlutrans.h": {
        "m2t_transblock_train_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
        "m2t_transblock_train_workspace_offset": (C.c_size_t, [_i, _i, _i, _i]),
        "m2t_transblock_forward_train": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
        "m2t_transblock_backward": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    },
    "m2t_infer.h": {
        "m2t_dihedral_pack": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
        "m2t_dihedral_merge": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
        "m2t_tensor_to_image_u8": (_i, [_vp, _i, _i, _i, _f, _vp, _vp]),
    },
    "m2t_train.h": {
        "m2t_meter_reset": (_i, [_vp, _vp, _i, _i, _vp]),
        "m2t_meter_update": (_i, [C.POINTER(_vp), C.POINTER(_i), _i, _vp, _vp, _i, _ll, _vp]),
        "m2t_preview_strip": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    },
    "m2t_tiles.h": {
        "m2t_tile_grid": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
        "m2t_tile_gather": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
        "m2t_tile_blend": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    },
    "m2t_gmsd.h": {
        "m2t_gmsd_loss_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i]),
        "m2t_gmsd_loss_tensor": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _i, _f, _i, _d, _vp, _vp, _vp, _i, _vp, _vp]),
        "m2t_gmsd_loss": (_i, [_vp, _vp, _f, _d, _f, _vp, _i, _vp, _vp, _vp]),
    },
    "m2t_degrade.h": {
        "m2t_degrade_patches": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _ull, _vp, _vp, _vp]),
        "m2t_degrade_image_u8": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i, _ull, _ull, _d, _d, _i, _vp, _vp]),
    },
    "m2t_jpeg.h": {
        "m2t_jpeg_quant_tables": (_i, [_i, C.POINTER(_i), C.POINTER(_i)]),
        "m2t_jpeg_image_u8": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp]),
        "m2t_degrade_jpeg_patches": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _ull, _vp, _vp, _vp]),
        "m2t_degrade_jpeg_image_u8": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i, _ull, _ull, _d, _d, _i, _vp, _i, _vp, _vp]),
    },
    "m2t_wavelet.h": {
        "m2t_wavelet_loss_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i]),
        "m2t_swt2": (_i, [_vp, _i, _i, _i, _i, _ll, _i, _dp, _dp, _i, _i, _vp, _vp, _vp]),
        "m2t_wavelet_loss_tensor": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _i, _f, _i, _d, _dp, _dp, _i, _i, _dp, _d, _vp, _vp, _vp, _i, _vp, _vp]),
        "m2t_wavelet_loss": (_i, [_vp, _vp, _f, _d, _f, _dp, _dp, _i, _i, _dp, _d, _vp, _i, _vp, _vp, _vp]),
    },
    "m2t_text.h": {
        "m2t_text_encode_ex": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), _i, _i, _vp, _vp, _vp, _vp]),
    },
    "m2t_swin.h": {
        "m2t_swin_encode_ex": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, C.POINTER(_i), _i, _vp, _vp, _vp, _vp]),
        "m2t_swin_backward_ex": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    },
    "m2t_consistency.h": {
        "m2t_consistency_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
        "m2t_imresize_adjoint_f32": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _vp]),
        "m2t_consistency_loss_tensor": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _ll, _i, _f, _i, _d, _d, _vp, _vp, _vp, _i, _vp, _vp]),
        "m2t_consistency_loss": (_i, [_vp, _vp, _f, _d, _f, _d, _vp, _i, _vp, _vp, _vp]),
        "m2t_back_project_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _d, _i, _vp, _vp, _vp]),
    },
}

# constants of the headers, by header
FFT_NORMS = {"backward": 0, "ortho": 1}     # the `norm` argument of the spectral entry points, by torch.fft's names

MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)     # the five level weights of the term
MSSSIM_MIN_SIDE = 161                                          # min(H, W) > 160 = (11 - 1) * 2^4

VIF_MIN_SIDE = 41                                              # min(H, W) >= 41: the scale-3 map is then 1 x 1
VIF_SIGMA_N_SQ = 2.0                                           # the default variance of the visual noise

MAX_GROUPS = 8                                                 # M2T_MAX_GROUPS
MAX_SEGMENTS = 1024                                            # M2T_MAX_SEGMENTS

VGG_MIN_SIDE = 16                                              # min(H, W) >= 16: relu5_1 is then 1 x 1
VGG_LAYERS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)  # torchvision vgg19: features.<i> of the 13 convolutions up to conv5_1
VGG_CHANNELS = (64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512)
VGG_LEVEL = (0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4)            # 2 x 2 pools before the layer
VGG_TAP_LAYERS = (0, 2, 4, 8, 12)                              # relu1_1, relu2_1, relu3_1, relu4_1, relu5_1

TRANSBLOCK_NPARAMS = 22928                                     # TransBlock(n_feat=64, dim=64), state_dict order
TRANSBLOCK_REGIONS = {"H1": 0, "AO": 1, "weights": 2, "X": 3, "LN1": 4, "R": 5, "QKV": 6, "X1": 7, "LN2": 8}

METER_MAX_COLS = 16                                            # M2T_METER_MAX_COLS
METER_RECORD = ("sum", "count", "nonfinite", "min", "max", "last")     # the first six of the 8 doubles of a column

GMSD_MIN_SIDE = 2                                              # min(H, W) >= 2: one 2 x 2 cell

DEGRADE_DESC_COLS = 11                                         # M2T_DEGRADE_DESC_COLS
DEGRADE_KMAX = {2: 20, 3: 21, 4: 20}                           # the largest K per scale; K has the parity of the scale

JPEG_DESC_COLS = 12                                            # M2T_DEGRADE_JPEG_DESC_COLS: column 11 is the quality
JPEG_CONSTS = 320                                              # M2T_JPEG_CONSTS: T[64], recip[256]

WAVELET_MAX_TAPS, WAVELET_MAX_LEVELS = 8, 3


def wavelet_min_side(taps: int, levels: int) -> int:
    """min(H, W) the wavelet entries take: a tap index wraps at most once."""
    return (int(taps) - 1) * 2 ** (int(levels) - 1) + 1


_lib = None


class M2TError(RuntimeError):
    pass


def load():
    """Load libm2t.so once; raises M2TError when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise M2TError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m m2trans_amd.build` "
            "(needs hipcc). There is no CPU fallback for this path.")
    # torch must bring in ITS HIP runtime (torch/lib/libamdhip64.so) first: libm2t.so then binds
    # to that already-loaded runtime, so streams and device pointers are shared with torch.
    # Loaded the other way round the process ends up with two runtimes (and ours sees no device).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for table in ABI.values():
        for name, (res, args) in table.items():
            fn = getattr(lib, name)          # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().m2t_last_error_string()
        raise M2TError(f"{what} failed with status {rc}: {msg.decode() if msg else ''}")


class Handle:
    """What every owner of a library handle of ``family`` (m2t_<family>_create: plan, swin, text, vgg) shares: ``query``, the
    parameter inventory, and the destroy call when the owner goes.  The owner sets ``self.handle``."""
    family = ""
    handle = None

    def query(self, key: str) -> int:
        v = getattr(load(), f"m2t_{self.family}_query")(self.handle, key.encode())
        if v < 0:
            raise KeyError(key)
        return int(v)

    def inventory(self):
        """(names in flat order, {name: (float offset, element count)}) of the flat parameter buffer, as the library lays it"""
        name = getattr(load(), f"m2t_{self.family}_param_name")
        names = [name(self.handle, i).decode() for i in range(self.query("num_param_tensors"))]
        return names, {n: (self.query("param:" + n), self.query("numel:" + n)) for n in names}

    def __del__(self):
        try:
            if self.handle:
                getattr(load(), f"m2t_{self.family}_destroy")(self.handle)
                self.handle = None
        except Exception:
            pass


def ptr(t):
    """Device/host pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
