"""ctypes binding of librcot_hip.so (C ABI declared in include/rcot_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol is
absent, importing/using the kernels raises immediately (``RcotLibraryError``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 42    # == RCOT_ABI_VERSION in include/rcot_hip.h (checked by tests/test_abi.py and at load time)
PREC_FP32, PREC_BF16X3, PREC_BF16X6, PREC_BF16X1 = 0, 1, 2, 3     # RCOT_PREC_* of include/rcot_hip.h
# the control block of a guarded optimizer (include/rcot_hip.h): word indices into a float64 tensor of CB_WORDS (the I words through .view(int64))
SUMSQ_MAX_PARTS, CB_WORDS = 4096, 16
DECIDE_ADAM0, DECIDE_ADAM1, DECIDE_INHERIT = 1, 2, 4               # flags of rcot_grad_decide
CB_LR, CB_MAX_NORM, CB_NORM, CB_SCALE, CB_STEPS, CB_CLIPPED, CB_SKIPPED, CB_MAX_SEEN, CB_SKIP, CB_T, CB_BC1, CB_BC2 = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13
# the schedule block of rcot_sched_advance (include/rcot_hip.h RCOT_SB_*): word indices into a float64 tensor of SB_WORDS
SB_WORDS, SB_T, SB_LR, SB_EMA_UPDATES, SB_EMA_DECAY, SB_EMA_OMD = 8, 0, 1, 2, 3, 4
LIB_PATH = os.environ.get("RCOT_LIB") or os.path.join(_HERE, "librcot_hip.so")   # RCOT_LIB: A/B builds while tuning


class RcotLibraryError(RuntimeError):
    pass


class RcotKernelError(RuntimeError):
    pass


_f = C.c_void_p          # device pointers travel as integers
_l = C.c_long
_i = C.c_int
_fl = C.c_float
_d = C.c_double
_sz = C.c_size_t

class KmajorDesc(C.Structure):
    """rcot_kmajor_desc of include/rcot_hip.h (one product of rcot_gemm_kmajor_multi)"""
    _fields_ = [("At", _f), ("lda", _l), ("sAo", _l), ("sAi", _l), ("a_rows", _i),
                ("Bm", _f), ("ldb", _l), ("sBo", _l), ("sBi", _l),
                ("C", _f), ("ldc", _l), ("sCo", _l), ("sCi", _l),
                ("R", _f), ("ldr", _l), ("sRo", _l), ("sRi", _l),
                ("rowscale", _f), ("sSo", _l), ("sSi", _l),
                ("Zo", _i), ("Zi", _i), ("M", _i), ("K", _i)]


# name -> argtypes, mirroring include/rcot_hip.h exactly (order matters)
SIGNATURES = {
    "rcot_abi_version": [],
    "rcot_last_kernel": [_f, _i],            # char* out: a ctypes string buffer
    "rcot_debug_nt_coop": [_i],              # host-side test hook (no launch)
    "rcot_profile_begin": [],
    "rcot_profile_end": [_f, _i],            # char* out: a ctypes string buffer
    "rcot_conv1x1_fwd": [_f, _l, _f, _l, _f, _l, _i, _i, _i, _i, _f, _f, _f, _f, _f, _l, _fl, _f],
    "rcot_conv1x1_dgrad": [_f, _l, _f, _l, _f, _l, _i, _i, _i, _i, _fl, _f],
    "rcot_conv1x1_wgrad": [_f, _l, _f, _l, _f, _l, _i, _i, _i, _i, _f, _f, _f, _f, _fl, _f, _sz, _i, _f],
    "rcot_conv1x1_wgrad_slabs": [_f, _l, _f, _l, _i, _i, _i, _i, _f, _f, _f, _f, _f, _sz, _i, _f, _f, _f],   # int* S, int* ldws: HOST
    "rcot_conv1x1_dgrad_wgrad_slabs": [_f, _l, _f, _f, _l, _f, _l, _f, _l, _i, _i, _i, _i, _f, _f, _f, _f, _f, _sz, _f, _sz, _i, _f, _f, _f],   # int* S, int* ldws: HOST
    "rcot_bmm_nn": [_f, _l, _l, _l, _i, _f, _l, _l, _l, _f, _l, _l, _l, _f, _l, _l, _l, _f, _l, _l,
                    _i, _i, _i, _i, _i, _fl, _f],
    "rcot_bmm_nt": [_f, _l, _l, _l, _f, _l, _l, _l, _f, _l, _l, _l, _i, _i, _i, _i, _i, _f, _sz, _i, _f],
    "rcot_bmm_nt_slabs": [_f, _l, _l, _l, _f, _l, _l, _l, _i, _i, _i, _i, _i, _f, _sz, _i, _f, _f, _f],   # int* S, int* ldws: HOST
    "rcot_gemm_kmajor": [_f, _l, _l, _l, _i, _f, _l, _l, _l, _f, _l, _l, _l, _f, _l, _l, _l, _f, _l, _l,
                         _f, _f, _l, _i, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _fl, _f, _sz, _i, _f],
    "rcot_gemm_kmajor_stats": [_f, _l, _l, _l, _i, _f, _l, _l, _l, _f, _l, _l, _l, _f, _l, _l, _l, _f, _f, _l, _i, _i, _i, _i, _i, _f],
    "rcot_kmajor_desc_size": [],
    "rcot_gemm_kmajor_multi": [_f, _i, _i, _i, _f],         # rcot_kmajor_desc* d: a HOST ctypes array of KmajorDesc
    "rcot_pack_weight": [_f, _l, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f],
    "rcot_pack_weights": [_f, _f, _i, _f],
    "rcot_linear_fwd": [_f, _f, _f, _f, _i, _i, _i, _fl, _f, _sz, _f],
    "rcot_linear_dgrad": [_f, _f, _f, _i, _i, _i, _f, _sz, _f],
    "rcot_linear_wgrad": [_f, _f, _f, _i, _i, _i, _fl, _f],
    "rcot_conv2d_fwd": [_f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _i, _fl, _i, _f, _f, _fl, _f, _sz, _f],
    "rcot_conv2d_dgrad": [_f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _i, _fl, _f, _fl, _f, _sz, _f],
    "rcot_conv2d_wgrad": [_f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _i, _fl, _f, _sz, _f],
    "rcot_conv_pcm_prep": [_f, _f, _l, _i, _i, _i, _i, _i, _f],
    "rcot_conv_pcm_wgrad": [_f, _f, _l, _i, _i, _i, _i, _f, _fl, _f, _sz, _i, _f],
    "rcot_conv_pcm_merge": [_f, _l, _f, _i, _i, _i, _i, _f],
    "rcot_conv_pcm_pack": [_f, _f, _f, _i, _i, _f, _f],
    "rcot_conv_pcm": [_f, _i, _i, _f, _l, _i, _f, _i, _f, _fl, _f, _f, _l, _f, _sz, _f],   # tapoff: HOST int array
    "rcot_pixel_shuffle": [_f, _f, _l, _i, _i, _i, _f],
    "rcot_ln_stats": [_f, _f, _f, _i, _i, _i, _f],
    "rcot_ln_bwd": [_f, _f, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i, _f, _l, _f],
    "rcot_ln_bwd_rows": [_i, _i, _i],
    "rcot_block_param_reduce": [_f, _f, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _i, _i, _f, _i, _f],   # slab_sets: HOST array
    "rcot_slab_sets_reduce": [_f, _i, _f],                                                            # slab_sets: HOST array
    "rcot_dwconv3x3": [_f, _f, _f, _i, _i, _i, _i, _i, _f],
    "rcot_gdfn_gate_fwd": [_f, _f, _f, _i, _i, _i, _i, _f],
    "rcot_gdfn_gate_bwd": [_f, _f, _f, _f, _f, _i, _i, _i, _i, _f],
    "rcot_gdfn_bwd": [_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _f],
    "rcot_dwconv3x3_wgrad": [_f, _f, _f, _i, _i, _i, _i, _f],
    "rcot_dwconv3x3_bwd": [_f, _f, _f, _f, _f, _i, _i, _i, _i, _f],
    "rcot_row_sumsq": [_f, _f, _i, _i, _i, _l, _f],
    "rcot_attn_softmax": [_f, _i, _i, _f, _f, _f, _f, _i, _i, _i, _f],
    "rcot_attn_bwd_small": [_f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i, _f],
    "rcot_attn_core_fwd": [_f, _l, _f, _f, _l, _f, _f, _f, _f, _l, _l, _i, _i, _i, _i, _f, _sz, _f],
    "rcot_attn_core_bwd": [_f, _i, _i] + [_f] * 12 + [_i, _i, _i, _f],
    "rcot_attn_rows_bwd": [_f, _i, _i] + [_f] * 12 + [_i, _i, _i, _i, _f, _sz, _f],
    "rcot_attn_rows_ws_bytes": [_i, _i, _i, _i],                                               # returns the byte count (no launch)
    "rcot_batch_reduce": [_f, _f, _i, _l, _fl, _f],
    "rcot_lrelu_bwd": [_f, _f, _f, _l, _fl, _f],
    "rcot_bias_grad": [_f, _f, _i, _i, _i, _f],
    "rcot_axpby2d": [_f, _l, _f, _l, _f, _l, _l, _l, _fl, _fl, _f],
    "rcot_fill": [_f, _l, _fl, _f],
    "rcot_lerp": [_f, _f, _f, _f, _i, _l, _f],
    "rcot_gp_penalty": [_f, _f, _f, _f, _i, _l, _fl, _f],
    "rcot_ot_reduce": [_f, _f, _f, _f, _i, _l, _f],
    "rcot_fft_plan": [_i, _f, _i],           # int* radices: a HOST ctypes int array (no launch)
    "rcot_ot_spectrum": [_f, _f, _f, _f, _f, _f, _sz, _i, _i, _i, _f],
    "rcot_ot_grad": [_f, _f, _f, _f, _f, _f, _f, _f, _f, _i, _l, _fl, _fl, _l, _f],
    "rcot_patch_prep": [_f, _f, _i, _i, _i, _i, _i, _i, _fl, C.c_ulonglong, _f, _f, _f],
    "rcot_patch_prep_batch": [_f, _i, _i, _f, _f, _f],                                         # table: a DEVICE int64 array
    "rcot_rmsprop_step": [_f, _f, _f, _l, _d, _d, _d, _d, _f],
    "rcot_adam_step": [_f, _f, _f, _f, _l, _d, _d, _d, _d, _i, _d, _f],
    "rcot_ema_step": [_f, _f, _l, _d, _f],
    # gradient-norm clipping / non-finite skip decided on the device (control block: RCOT_CB_* below)
    "rcot_grad_sumsq_parts": [_l],                                                             # returns the count (no launch)
    "rcot_grad_sumsq": [_f, _l, _f, _f],
    "rcot_grad_decide": [_f, _i, _f, _i, _d, _d, _f],
    "rcot_rmsprop_step_guarded": [_f, _f, _f, _l, _d, _d, _f, _f],
    "rcot_adam_step_guarded": [_f, _f, _f, _f, _l, _d, _d, _d, _f, _i, _f],
    # AdamW (decoupled weight decay), the schedule block's advance launch and the EMA step that reads 1 - decay from a device word
    "rcot_adamw_step": [_f, _f, _f, _f, _l, _d, _d, _d, _d, _i, _d, _d, _f],
    "rcot_adamw_step_guarded": [_f, _f, _f, _f, _l, _d, _d, _d, _f, _i, _d, _f],
    "rcot_sched_advance": [_f, _f, _i, _f, _d, _f, _d, _f],
    "rcot_ema_step_dev": [_f, _f, _l, _f, _f],
    # the MPRNet backbone's pointwise pieces (csrc/mprnet_ops.hip)
    "rcot_prelu_fwd": [_f, _f, _f, _l, _f],
    "rcot_prelu_bwd": [_f, _f, _f, _f, _f, _l, _f, _sz, _f],
    "rcot_row_dot": [_f, _f, _f, _l, _i, _fl, _f],
    "rcot_row_scale_add": [_f, _f, _f, _f, _fl, _f, _l, _i, _f],
    "rcot_ca_gate_fwd": [_f, _f, _f, _f, _f, _i, _i, _i, _f],
    "rcot_ca_gate_bwd": [_f, _f, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i, _f, _sz, _f],
    "rcot_bilinear_down2": [_f, _f, _l, _i, _i, _f],
    "rcot_bilinear_down2_bwd": [_f, _f, _l, _i, _i, _fl, _f],
    "rcot_bilinear_up2": [_f, _f, _f, _l, _i, _i, _f],
    "rcot_bilinear_up2_bwd": [_f, _f, _l, _i, _i, _f],
    "rcot_conv_weight_flip": [_f, _f, _f, _i, _i, _i, _i, _i, _f],
    # whole-image validation at any size (csrc/imageio.hip)
    "rcot_image_ingest": [_f, _i, _i, _f, _i, _i, _i, _f],
    "rcot_pad2d": [_f, _f, _l, _i, _i, _i, _i, _i, _f],
    "rcot_image_egress": [_f, _f, _f, _i, _i, _i, _i, _fl, _f, _f, _f, _f, _sz, _f],
    "rcot_image_ingest_batch": [_f, _i, _i, _i, _i, _f, _f],                                   # table: a DEVICE int64 array
    "rcot_image_egress_batch": [_f, _f, _i, _i, _i, _f, _f, _sz, _f],                          # table: a DEVICE int64 array
    # standard image-quality figures (csrc/quality.hip)
    "rcot_image_quality": [_f, _f, _i, _i, _i, _i, _f, _f, _sz, _f],
    "rcot_image_blockiness": [_f, _f, _i, _i, _i, _i, _i, _f, _f, _sz, _f],                    # stats: a DEVICE int64 array
    "rcot_crop_u8": [_f, _i, _i, _i, _i, _i, _i, _f, _f],
    # views of an image and their weighted blend: tiles and the x8 self-ensemble (csrc/views.hip)
    "rcot_view_gather": [_f, _i, _i, _i, _f, _i, _f, _i, _f, _i, _i, _i, _f, _f],             # ys, xs, modes: HOST int arrays
    "rcot_view_blend": [_f, _i, _i, _i, _f, _i, _f, _i, _f, _i, _i, _i, _f, _f, _f, _f],       # ys, xs, modes: HOST int arrays
    # MATLAB-rule bicubic resize, one axis per launch (csrc/resize.hip)
    "rcot_resize_axis": [_f, _f, _l, _i, _i, _i, _i, _f, _f, _i, _f],                          # idx, taps: DEVICE arrays
    # baseline JPEG round trip (csrc/jpeg.hip)
    "rcot_jpeg_ws_bytes": [_i, _i, _i],                                                        # returns the byte count (no launch)
    "rcot_jpeg_roundtrip": [_f, _f, _i, _i, _i, _i, _f, _sz, _f],
    # per-image PSF blur (csrc/blur.hip)
    "rcot_blur_u8": [_f, _f, _i, _i, _f, _i, _i, _i, _i, _f],                                  # psf: a DEVICE int32 array
    # whole-image noise (csrc/noise.hip)
    "rcot_noise_u8": [_f, _f, _i, _i, _i, _fl, _fl, C.c_ulonglong, _f],
}

_lib = None


def load():
    """Load librcot_hip.so once.  ``import torch`` happens first so the HIP runtime
    (libamdhip64.so.7) already mapped by torch is the one our library binds to."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (maps libamdhip64 / librccl before we dlopen)
    if not os.path.isfile(LIB_PATH):
        raise RcotLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C rcot_amd/csrc`. There is no CPU/PyTorch fallback for the RCOT hot path.")
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise RcotLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RcotLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.argtypes = argtypes
        fn.restype = C.c_int
    if lib.rcot_abi_version() != ABI_VERSION:
        raise RcotLibraryError("librcot_hip.so ABI version mismatch")
    _lib = lib
    return lib


EUNSUPPORTED = -3     # RCOT_EUNSUPPORTED: the entry point has no kernel for the shape (callers fall back to the general one)


def check(rc: int, what: str):
    if rc == 0:
        return
    if rc == EUNSUPPORTED:
        raise RcotKernelError(f"{what}: no kernel for this shape")
    if rc == -1:
        raise RcotKernelError(f"{what}: invalid argument (shape/alignment/null)")
    if rc == -2:
        raise RcotKernelError(f"{what}: workspace too small")
    raise RcotKernelError(f"{what}: HIP error {rc}")
