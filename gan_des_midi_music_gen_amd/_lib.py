"""ctypes binding of libgdm_hip.so (C ABI: include/gdm.h).  No fallback: a missing library is a hard error."""
import ctypes
import os
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
# GDM_LIB_TAG=<tag>: load an experiment build (build.py, GDM_BUILD_TAG) instead of the shipped library; such a build
# reports gdm_build_flavor() == 1 and bench.py refuses it.
_TAG = os.environ.get("GDM_LIB_TAG", "")
LIB_PATH = os.path.join(_PKG, "libgdm_hip" + (f"_{_TAG}" if _TAG else "") + ".so")

F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3
# model 2's criterion names -> GDM_CRIT_* (include/gdm.h; network_tests.py:248-250 of the reference)
CRITERIA = {"bce": 0, "mse": 1, "l1": 2}
# GDM_PCM_* sample formats (include/gdm.h) and their bytes per sample
PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32 = range(5)
PCM_BYTES = (1, 2, 3, 4, 4)

_c = ctypes
_P, _I, _L, _F, _Z = _c.c_void_p, _c.c_int, _c.c_int64, _c.c_float, _c.c_size_t

class LinearBnJob(_c.Structure):
    """gdm_linear_bn_job (include/gdm.h)."""
    _fields_ = [(n, _P) for n in ("x", "w", "bias", "gamma", "beta", "running_mean", "running_var",
                                  "num_batches_tracked", "y_out", "out", "save_mean", "save_invstd")] + \
               [(n, _I) for n in ("M", "N", "K", "groups", "stat_repeats")]


class DcnnAdam(_c.Structure):
    """gdm_dcnn_adam (include/gdm.h)."""
    _fields_ = [("param", _P * 6), ("exp_avg", _P * 6), ("exp_avg_sq", _P * 6), ("hyper", _P), ("done", _P)]


class ConcatJob(_c.Structure):
    """gdm_concat_job (include/gdm.h)."""
    _fields_ = [("a", _P), ("b", _P), ("out", _P), ("M", _I), ("Ka", _I), ("Kb", _I)]


class MmganGenEvalJob(_c.Structure):
    """gdm_mmgan_gen_eval_job (include/gdm.h)."""
    _fields_ = [("noise", _P), ("input", _P), ("pack", _P), ("pack_bytes", _Z), ("out", _P), ("tap_y", _P * 4),
                ("tap_a", _P * 3)] + [(n, _I) for n in ("B", "z", "in_", "input_stride", "n4")]


# name -> (restype, argtypes); must list every function declared in include/gdm.h (tests/test_abi.py checks that)
SIGNATURES = {
    "gdm_last_error": (_c.c_char_p, []),
    "gdm_version": (_I, []),
    "gdm_arch": (_c.c_char_p, []),
    "gdm_build_flavor": (_I, []),
    "gdm_gemm": (_I, [_P, _I, _L, _L, _P, _I, _L, _L, _P, _I, _L, _L, _I, _I, _I, _P, _P, _I, _F, _I, _I, _P, _Z, _P]),
    "gdm_gemm_plan": (_I, [_P, _I, _L, _L, _P, _I, _L, _L, _P, _I, _L, _L, _I, _I, _I, _P, _I, _I, _P]),
    "gdm_bce_with_logits": (_I, [_P, _F, _I, _F, _P, _P, _I, _I, _P]),
    "gdm_criterion_loss": (_I, [_P, _F, _I, _I, _F, _P, _P, _I, _P]),
    "gdm_adam_step": (_I, [_P, _P, _P, _P, _L, _I, _F, _F, _F, _F, _F, _P]),
    "gdm_adam_step_dev": (_I, [_P, _P, _P, _P, _L, _P, _P]),
    "gdm_adam_step_dev_pc": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _I, _P]),
    "gdm_stft_frames": (_I, [_P, _I, _L, _L, _I, _I, _I, _P, _P]),
    "gdm_power_spectrum": (_I, [_P, _L, _I, _I, _P, _P]),
    "gdm_power_to_db": (_I, [_P, _I, _I, _I, _F, _F, _P, _P]),
    "gdm_pcm_to_float": (_I, [_P, _I, _I, _I, _L, _L, _L, _P, _P]),
    "gdm_pcm_stft_frames": (_I, [_P, _I, _I, _I, _L, _L, _L, _I, _L, _L, _I, _I, _I, _P, _P]),
    "gdm_bn_workspace_bytes": (_Z, [_I, _I]),
    "gdm_bn_act_fwd": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _F, _F, _I, _P, _I, _P, _P, _I, _P, _Z, _P]),
    "gdm_bn_act_bwd": (_I, [_P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _Z, _P]),
    "gdm_bn_stats": (_I, [_P, _I, _I, _P, _P, _P, _F, _F, _P, _P, _P, _Z, _P]),
    "gdm_bn_partial_chunks": (_I, [_I]),
    "gdm_bn_partials": (_I, [_P, _I, _I, _P, _P]),
    "gdm_bn_apply": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _P, _I, _P]),
    "gdm_bn_finalize": (_I, [_P, _I, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P]),
    "gdm_simnn_gen_pack_bytes": (_Z, []),
    "gdm_simnn_gen_pack": (_I, [_P, _I, _P, _P, _P, _P]),
    "gdm_simnn_gen_first": (_I, [_P, _I, _I, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P]),
    "gdm_simnn_gen_convt_chunks": (_I, [_I, _I]),
    "gdm_simnn_gen_convt_bn": (_I, [_I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "gdm_simnn_gen_last": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "gdm_simnn_gen_eval": (_I, [_P, _I, _I, _P, _P] + [_P] * 12 + [_F, _P, _P, _P, _P, _P, _P]),
    "gdm_bias_act_fwd": (_I, [_P, _P, _I, _I, _I, _F, _P, _I, _P]),
    "gdm_act_bwd": (_I, [_P, _P, _I, _L, _I, _F, _P, _P]),
    "gdm_colsum": (_I, [_P, _I, _I, _I, _P, _P, _Z, _P]),
    "gdm_cast": (_I, [_P, _I, _P, _I, _L, _P]),
    "gdm_nonfinite_count": (_I, [_P, _I, _L, _P, _P]),
    "gdm_simnn_conv1_fwd": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _P]),
    "gdm_simnn_conv1_fwd_pair": (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _P, _P, _I, _P]),
    "gdm_simnn_conv2_pack_bytes": (_Z, [_I]),
    "gdm_simnn_conv2_pack": (_I, [_P, _I, _P, _P]),
    "gdm_simnn_conv2_fwd": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _P]),
    "gdm_simnn_conv2_bwd_fused_workspace_bytes": (_Z, [_I, _I, _I]),
    "gdm_simnn_conv2_bwd_fused": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P, _I, _P, _Z, _P]),
    "gdm_simnn_conv2_bwd_fused_finish": (_I, [_I, _I, _I, _P, _P, _P, _Z, _P]),
    "gdm_simnn_conv2_bwd_data": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _P]),
    "gdm_simnn_conv2_bwd_weight_workspace_bytes": (_Z, [_I, _I, _I]),
    "gdm_simnn_conv2_bwd_weight": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _Z, _P]),
    "gdm_simnn_conv1_bwd_weight_workspace_bytes": (_Z, [_I, _I, _I]),
    "gdm_simnn_conv1_bwd_weight": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _P, _Z, _P]),
    "gdm_simnn_conv1_bwd_data": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _P]),
    "gdm_simnn_adam_step": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P]),
    "gdm_simnn_head_workspace_bytes": (_Z, [_I]),
    "gdm_simnn_head": (_I, [_P, _P, _P, _I, _I, _F, _F, _P, _P, _I, _P, _I, _P, _P, _P, _P, _Z, _P]),
    "gdm_linear_bn_act_max_rows": (_I, []),
    "gdm_linear_bn_act_fwd_multi": (_I, [_P, _I, _F, _F, _I, _I, _P]),
    "gdm_concat_cols_multi": (_I, [_P, _I, _P]),
    "gdm_linear_bn_act_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _F, _F, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I,
                                   _P]),
    "gdm_dcnn_fused_supported": (_I, [_I]),
    "gdm_dcnn_pack_bytes": (_Z, [_I]),
    "gdm_dcnn_pack": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "gdm_dcnn_fused_workspace_bytes": (_Z, [_I, _I, _I]),
    "gdm_dcnn_fused": (_I, [_P, _I, _P, _P, _I, _I, _F, _F, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "gdm_dcnn_fused_adam": (_I, [_P, _I, _P, _P, _I, _I, _F, _F, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "gdm_dcnn_fused_crit": (_I, [_P, _I, _P, _P, _I, _I, _F, _F, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _Z,
                                 _P]),
    "gdm_dcnn_fused_adam_crit": (_I, [_P, _I, _P, _P, _I, _I, _F, _F, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P,
                                      _Z, _P]),
    "gdm_mmgan_gen_eval_supported": (_I, [_I, _I, _I, _I, _I]),
    "gdm_mmgan_gen_eval_pack_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "gdm_mmgan_gen_eval_pack": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _Z, _P]),
    "gdm_mmgan_gen_eval": (_I, [_P, _I, _I, _I, _I, _P]),
    "gdm_im2col": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "gdm_col2im": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _I, _P]),
    "gdm_permute_pc": (_I, [_P, _I, _I, _I, _I, _P, _I, _P]),
    "gdm_des_scan": (_I, [_P, _L, _I, _I, _I, _F, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "gdm_des_routing": (_I, [_P, _L, _I, _I, _I, _P, _P, _P, _P]),
    "gdm_des_draws": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I] + [_P] * 16),
    "gdm_des_draws_host": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I] + [_P] * 15),
    "gdm_des_run": (_I,[_P, _I, _P, _P, _P, _L, _L, _L, _P, _P, _P, _P, _P, _L, _P, _P]),
    "gdm_des_batch_workspace_bytes": (_L, [_I, _I, _I]),
    "gdm_des_pack": (_I, [_I, _L, _P, _P, _P, _P, _P, _P, _P]),
    "gdm_des_math_probe_host": (_I, [_P, _L, _P, _P]),
    "gdm_des_math_probe": (_I, [_P, _L, _P, _P, _P]),
    "gdm_des_stats_workspace_bytes": (_L, [_I, _I, _I]),
    "gdm_des_log_tracks_count": (_I, [_P, _P, _P, _L, _I, _I, _P, _L, _P, _P, _P, _P]),
    "gdm_des_log_tracks": (_I, [_P, _P, _P, _L, _I, _I, _P, _I, _L, _P, _L, _P, _P]),
    "gdm_des_log_tracks_host": (_I, [_P, _P, _P, _L, _I, _I, _P, _I, _L, _P, _P, _P, _P, _L]),
    "gdm_des_log_visits_host": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _L]),
    "gdm_piano_roll_raster": (_I, [_P, _P, _P, _I, _I, _P, _P, _P]),
    "gdm_piano_roll_windows": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "gdm_des_log_to_roll": (_I, [_P, _P, _P, _P, _P, _L, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P,
                                 _P]),
    "gdm_des_log_to_notes": (_I, [_P, _P, _P, _P, _P, _L, _P, _I, _I, _P, _I, _P, _P, _P, _P]),
    "gdm_synth_frames": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P]),
    "gdm_synth_pcm": (_I, [_P, _I, _P, _P, _P, _L, _L, _P, _P]),
    "gdm_synth_windows": (_I, [_P, _P, _L, _P, _I, _P, _P, _I, _L, _L, _P, _P, _P, _P]),
    "gdm_s2w_prologue": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gdm_des_log_to_notes_pc": (_I, [_P, _P, _P, _P, _P, _L, _P, _P, _I, _I, _L, _L, _L, _P, _I, _P, _P, _P, _P]),
    "gdm_synth_windows_gm": (_I, [_P, _P, _L, _P, _I, _P, _P, _I, _L, _L, _P, _P, _P, _P, _P]),
    "gdm_maxpool2_fwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "gdm_maxpool2_bwd": (_I, [_P, _I, _P, _I, _I, _I, _I, _P, _P]),
}

# The twelve batch entries of the DES simulator, gdm_des_{run,stats}_batch[_dist|_net][_host] (include/gdm.h), composed
# from the pieces of their argument lists:
_DES_NET = [_P, _I, _I, _P, _P]                        # adj, B, dim, loc, scale
_DES_KIND = [_P]                                       # kind (B, dim): the _dist and _net entries, behind scale
_DES_SPEC = [_P, _P, _P, _I]                           # queue_cap, seed, number_of_customers, max_queue_cap
_DES_MATH = [_I]                                       # math: the _host entries
_DES_CAPS = {"run": [_L, _L], "stats": [_L]}           # max_events; the log mode: max_records
_DES_STATE = [_P] * 4                                  # mt_key, mt_pos, has_gauss, cached_gauss
_DES_OUT = {"run": [_P, _P, _P, _P, _L, _P, _P, _P],   # value, event_id, node, kind, n_records_cap, rec_ptr, n_records,
                                                       # stop_reason
            "stats": [_P] * 15}                        # eight (B, dim) rows, six (B) rows, queue_time
_DES_DEVICE = [_P, _Z, _P]                             # workspace, workspace_bytes, stream: the device entries
for _mode in ("run", "stats"):
    for _policy in ("", "_dist", "_net"):
        for _host in ("", "_host"):
            SIGNATURES[f"gdm_des_{_mode}_batch{_policy}{_host}"] = (
                _I, _DES_NET + (_DES_KIND if _policy else []) + _DES_SPEC + (_DES_MATH if _host else []) +
                _DES_CAPS[_mode] + _DES_STATE + _DES_OUT[_mode] + ([] if _host else _DES_DEVICE))

# the host snapshot entry (des::SnapStats): the _net statistics list with snap_customers (B, S) and S in the place of
# number_of_customers
SIGNATURES["gdm_des_stats_batch_snap_host"] = (
    _I, _DES_NET + _DES_KIND + [_P, _P, _P, _I, _I] + _DES_MATH + _DES_CAPS["stats"] + _DES_STATE + _DES_OUT["stats"])

_lock = threading.Lock()
_lib = None


class GdmError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle; raises if libgdm_hip.so has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise GdmError(
                    f"{LIB_PATH} is missing: build it with `python -m gan_des_midi_music_gen_amd.build` "
                    "(hipcc --offload-arch=gfx950). There is no CPU or eager-PyTorch fallback for this path.")
            # PyTorch-ROCm ships its own libamdhip64: it must be in the process BEFORE this library's dependency on
            # libamdhip64.so is resolved, or the process ends up with two HIP runtimes and our kernels are registered
            # with the one that owns no device ("no ROCm-capable device is detected" on the first launch).
            import torch  # noqa: F401
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)  # AttributeError if the symbol is not exported
                fn.restype, fn.argtypes = res, args
            _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().gdm_last_error().decode(errors="replace")
        raise GdmError(f"{what} failed (rc={rc}): {msg}")
