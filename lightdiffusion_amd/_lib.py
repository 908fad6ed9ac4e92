"""ctypes binding of libld_mi355x.so (C ABI declared in include/ld_mi355x.h).

The product path has NO fallback: if the HIP library is missing, `lib()` raises — it never routes
to PyTorch eager or to the oracle.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LD_MI355X_LIB") or os.path.join(_HERE, "libld_mi355x.so")   # env: debug builds only

OK, ERR_ARG, ERR_SHAPE, ERR_HIP, ERR_STATE = 0, 1, 2, 3, 4
F16, F32 = 0, 1
FWD_EPS_ONLY, FWD_PAIR = 1, 2      # LD_FWD_*: the flags of ld_unet_forward / ld_controlnet_forward and their profiles


class UNetConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("model_channels", C.c_int), ("num_levels", C.c_int),
                ("channel_mult", C.c_int * 8), ("num_res_blocks", C.c_int * 8), ("transformer_depth", C.c_int * 16),
                ("transformer_depth_output", C.c_int * 24), ("transformer_depth_middle", C.c_int),
                ("context_dim", C.c_int), ("num_heads", C.c_int)]


class VAEConfig(C.Structure):
    _fields_ = [("z_channels", C.c_int), ("ch", C.c_int), ("num_levels", C.c_int), ("ch_mult", C.c_int * 8),
                ("num_res_blocks", C.c_int), ("out_ch", C.c_int), ("with_encoder", C.c_int)]


class ESRGANConfig(C.Structure):
    _fields_ = [("in_nc", C.c_int), ("out_nc", C.c_int), ("nf", C.c_int), ("gc", C.c_int), ("nb", C.c_int), ("scale", C.c_int)]


class LoraTerm(C.Structure):
    _fields_ = [("up", C.c_void_p), ("down", C.c_void_p), ("dtype", C.c_int), ("rank", C.c_int), ("scale", C.c_float)]


REGIONAL_MAX_ENTRIES = 16      # LD_REGIONAL_MAX_ENTRIES


class RegionalWindow(C.Structure):
    _fields_ = [("y0", C.c_int), ("x0", C.c_int)]


class RegionalEntry(C.Structure):
    _fields_ = [("out", C.c_void_p), ("mask", C.c_void_p), ("list", C.c_int), ("mask_batch", C.c_int), ("y0", C.c_int), ("x0", C.c_int),
                ("h", C.c_int), ("w", C.c_int), ("strength", C.c_float), ("mask_strength", C.c_float)]


CONTROL_MAX_SEGMENTS = 16      # residual slots of ld_control, segments of one ld_op_control_add


class Control(C.Structure):
    """ld_control"""
    _fields_ = [("residual", C.c_void_p * 16), ("count", C.c_int), ("middle", C.c_void_p), ("r_n", C.c_int), ("strength", C.c_float),
                ("c", C.c_int * 16), ("h", C.c_int * 16), ("w", C.c_int * 16)]


class LDError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        msg = lib().ld_status_string(status).decode() if _lib is not None else str(status)
        super().__init__(f"{where}: {msg} (status {status})")


_lib = None
_P, _I, _F, _Z = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# what every resident model exports alike, as ld_<family>_<op> (csrc/runtime.h `Model`)
_MODEL_OPS = {
    "destroy": (None, [_P]),
    "param_count": (_I, [_P]),
    "param_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_I), C.POINTER(C.c_int64)]),
    "load_param": (_I, [_P, C.c_char_p, _P, _I, _P]),
    "workspace_bytes": (_Z, [_P]),
    "last_launches": (_I, [_P]),
    "last_flops": (C.c_double, [_P]),
    "profile_launches": (_I, [_P, C.c_char_p, _Z]),
}
_SIZED_OPS = {"reserve": (_I, [_P, _I, _I, _I]), "plan_bytes": (_Z, [_P, _I, _I, _I])}   # (batch, h, w): all but the UNet, whose reserve adds the tokens

# name -> (restype, argtypes): every symbol include/ld_mi355x.h declares
SIGNATURES = {
    **{f"ld_{fam}_{op}": sig for fam in ("unet", "vae", "esrgan", "taesd") for op, sig in _MODEL_OPS.items()},
    **{f"ld_{fam}_{op}": sig for fam in ("vae", "esrgan", "taesd") for op, sig in _SIZED_OPS.items()},
    "ld_version": (C.c_char_p, []),
    "ld_status_string": (C.c_char_p, [_I]),
    "ld_unet_create": (_I, [C.POINTER(UNetConfig), C.POINTER(_P)]),
    "ld_unet_reserve": (_I, [_P, _I, _I, _I, _I]),
    "ld_unet_weight_bytes": (_Z, [_P]),
    "ld_unet_set_context": (_I, [_P, _P, _I, _I, _I, _P]),
    "ld_unet_forward": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, C.POINTER(Control), _P]),
    "ld_unet_profile": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, C.POINTER(Control), _P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_I)]),
    "ld_unet_profile_kernels": (_I, [_P, C.c_char_p, _Z]),
    "ld_unet_patch_param": (_I, [_P, C.c_char_p, C.POINTER(LoraTerm), _I, _P]),
    "ld_unet_unpatch": (_I, [_P, C.c_char_p, _P]),
    "ld_unet_read_param": (_I, [_P, C.c_char_p, _P, _P]),
    "ld_unet_refresh_derived": (_I, [_P, _P]),
    "ld_unet_patch_bytes": (_Z, [_P]),
    "ld_controlnet_create": (_I, [C.POINTER(UNetConfig), _I, C.POINTER(_P)]),
    "ld_controlnet_set_hint": (_I, [_P, _P, _I, _I, _I, _P]),
    "ld_controlnet_forward": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "ld_controlnet_residual_count": (_I, [_P]),
    "ld_controlnet_residual_batch": (_I, [_P]),
    "ld_controlnet_residual": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "ld_controlnet_read_residual": (_I, [_P, _I, _P, _P]),
    "ld_controlnet_read_hint": (_I, [_P, _P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _P]),
    "ld_controlnet_profile": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "ld_controlnet_fill_control": (_I, [_P, _I, _F, C.POINTER(Control)]),
    "ld_vae_create": (_I, [C.POINTER(VAEConfig), C.POINTER(_P)]),
    "ld_vae_decode": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "ld_vae_encode": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "ld_vae_profile": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "ld_vae_profile_encode": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "ld_esrgan_create": (_I, [C.POINTER(ESRGANConfig), C.POINTER(_P)]),
    "ld_esrgan_forward": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "ld_esrgan_profile": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "ld_taesd_create": (_I, [C.POINTER(_P)]),
    "ld_taesd_decode": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "ld_taesd_profile": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "ld_op_linear": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _F, _I, _P, _Z, _P]),
    "ld_op_linear_batched": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _F, _I, C.c_longlong, C.c_longlong, C.c_longlong, _P, _Z, _P]),
    "ld_op_conv": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "ld_op_vae_conv_out_takes_halo_tile": (_I, [_I, _I, _I, _I, _I]),
    "ld_op_groupnorm_conv_ws_bytes": (_Z, [_I, _I, _I, _I, _I, _I]),
    "ld_op_groupnorm_conv": (_I, [_P, _I, _P, _I, _I, _I, _I, _P, _P, _F, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _I, _P, _Z, _P]),
    "ld_op_repack_conv": (_I, [_P, _I, _I, _I, _P, _P]),
    "ld_op_upconv2x_fold": (_I, [_P, _I, _I, _P, _P]),
    "ld_op_upconv2x": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _Z, _P]),
    "ld_op_conv_skip_ws_bytes": (_Z, [_I, _I, _I, _I]),
    "ld_op_conv_skip": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _Z, _P]),
    "ld_op_groupnorm_conv_skip_ws_bytes": (_Z, [_I, _I, _I, _I, _I, _I, _I]),
    "ld_op_groupnorm_conv_skip": (_I, [_P, _I, _I, _I, _I, _P, _P, _F, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _Z, _P]),
    "ld_op_conv_takes_skip_segment": (_I, [_I, _I, _I, _I, _I]),
    "ld_op_groupnorm_ws_bytes": (_Z, [_I, _I]),
    "ld_op_groupnorm": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _F, _I, _P, _P, _P]),
    "ld_op_layernorm": (_I, [_P, _P, _P, _P, _I, _I, _F, _P]),
    "ld_op_attention": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _F, _I, _P]),
    "ld_op_conv_gn_partials_floats": (_Z, [_I, _I]),
    "ld_op_conv_gn_partials": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "ld_op_attention_rowv": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _F, _I, _P]),
    "ld_op_softmax_rows": (_I, [_P, _I, _I, _P]),
    "ld_op_timestep_embed": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "ld_op_cfg_combine": (_I, [_P, _P, _F, _Z, _P]),
    "ld_op_axpby": (_I, [_P, _F, _P, _F, _P, _F, _Z, _P]),
    "ld_op_hook_check": (_I, [_P, _P, _Z, _P, _Z, _P, _I, _P, _I, _P]),
    "ld_op_softmax_rows_ld": (_I, [_P, _I, _I, C.c_longlong, _I, _P]),
    "ld_op_groupnorm_chunks": (_I, [_I, _I]),
    "ld_op_groupnorm_stats": (_I, [_P, _I, _P, _I, _I, _I, _P, _P]),
    "ld_op_groupnorm_from_partials": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _F, _I, _P, _P, _I, _P]),
    "ld_op_groupnorm_scale_shift": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _F, _P, _I, _P, _P, _P]),
    "ld_op_small_conv_in": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, C.c_longlong, _P]),
    "ld_op_small_conv_out": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P]),
    "ld_op_small_pointwise": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "ld_op_vae_out_finish": (_I, [_P, _P, C.c_longlong, _I, _P]),
    "ld_op_timestep_embed_mod": (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _P]),
    "ld_op_dup_halves": (_I, [_P, _Z, _P, _Z, _P, _Z, _I, _P]),
    "ld_op_ctx_pad": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "ld_op_ctx_kv": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "ld_op_mlp_out_fold": (_I, [_P, _P, _P, _P, _I, _P, _P, _P]),
    "ld_op_ln_fold": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "ld_op_linear_ln": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P, _Z, _P]),
    "ld_op_linear_ln_geglu": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P, _Z, _P]),
    "ld_op_bislerp": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ld_op_esrgan_conv": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _F, _P, _I, _F, _P, _I, _F, _P]),
    "ld_op_esrgan_conv_y2": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _F, _P, _I, _F, _P, _I, _F, _P, _I, _P]),
    "ld_op_taesd_conv": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P]),
    "ld_op_esrgan_first": (_I, [_P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _P]),
    "ld_op_esrgan_last": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "ld_op_taesd_first": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "ld_op_taesd_last": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "ld_op_tile_blend": (_I, [_P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ld_op_last_kernel": (C.c_char_p, []),
    "ld_op_last_launches": (C.c_char_p, []),
    "ld_op_lora_merge": (_I, [_P, _P, _I, _I, C.POINTER(LoraTerm), _I, _P]),
    "ld_op_u8_resample": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _I, _P, _I, _P, _P]),
    "ld_op_u8_resample_tmp_bytes": (_Z, [_I, _I, _I]),
    "ld_op_u8_box_weights": (_I, [_F, C.POINTER(_I), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "ld_op_u8_blur_tmp_bytes": (_Z, [_I, _I]),
    "ld_op_u8_gaussian_blur": (_I, [_P, _I, _P, _I, _I, _I, _F, _P, _P]),
    "ld_op_u8_mask": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "ld_op_u8_composite": (_I, [_P, _I, _I, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ld_op_u8_from_f32": (_I, [_P, _P, _Z, _P]),
    "ld_op_f32_from_u8": (_I, [_P, _P, _Z, _P]),
    "ld_op_f32_crop_u8": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "ld_op_f32_blur_max_feather": (_I, []),
    "ld_op_f32_blur_tmp_bytes": (_Z, [_I, _I]),
    "ld_op_f32_gaussian_blur": (_I, [_P, _I, _P, _I, _I, _I, _I, _P, _P, _P]),
    "ld_op_f32_paste_u8": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "ld_op_inpaint_in": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ld_op_inpaint_out": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ld_op_regional_gather": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "ld_op_regional_combine": (_I, [_P, _I, _F, _P, _I, _I, _I, _I, _P]),
    "ld_op_control_add": (_I, [C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_longlong), _I, _I, _I, _F, _P]),
    "ld_op_hint_conv": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P]),
    "ld_op_clip_embed": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
}


def lib() -> C.CDLL:
    """Load (once) the in-tree HIP library; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              f"or `make -C lightdiffusion_amd/csrc`.  There is no CPU / PyTorch fallback for the hot path.")
        # Runtime resolution order: the library is linked against libamdhip64 without an rpath, so it binds to whichever HIP runtime the
        # process has loaded already, else to the loader's default (/opt/rocm/lib).  PyTorch ships its OWN libamdhip64: when torch is
        # present it must be loaded first — the other way round the process ends up with two HIP runtimes and the first hipMalloc here
        # fails (seen with build() + smoke() in one process).  A pure C-ABI / ctypes host without PyTorch gets the system runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        l = C.CDLL(LIB_PATH)
        missing = []
        for name, (res, args) in SIGNATURES.items():
            if not hasattr(l, name):
                if not os.environ.get("LD_MI355X_LIB"):
                    raise AttributeError(f"{LIB_PATH} does not export {name}: header and library out of sync — rebuild it")
                # an older commit's library named for a same-box comparison (tools/build_ref_lib.sh) has fewer entry points: a call of a
                # missing one fails with a clear message instead of an AttributeError deep inside ctypes.  (Not older than the flag form of
                # ld_unet_forward / ld_controlnet_forward: a symbol that is there is called with the signature above.)
                missing.append(name)
                setattr(l, name, _missing_symbol(name))
                continue
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        l._ld_missing = tuple(missing)
        _lib = l
    return _lib


def _missing_symbol(name: str):
    def fail(*_a, **_k):
        raise RuntimeError(f"{LIB_PATH} (LD_MI355X_LIB) does not export {name}: it was built from a commit without this entry point")
    return fail


def check(status: int, where: str) -> None:
    if status != OK:
        raise LDError(status, where)
