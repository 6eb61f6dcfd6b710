"""ctypes binding of include/gtcrn_micro_hip.h (the C-ABI drop-in boundary).

The product path is HIP only: if the shared library is missing, or no gfx950
device is present, everything here raises -- there is no CPU fallback and
nothing under oracle/ is ever imported from this package.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgtcrn_micro_hip.so")
NPARAM_FLOATS = 44938
NBINS = 257

_c_f32p = ctypes.POINTER(ctypes.c_float)
_vp = ctypes.c_void_p
_lib = None


class GtcrnError(RuntimeError):
    pass


def lib():
    """Loads libgtcrn_micro_hip.so (built in-tree by gtcrn_micro_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH
    variant = os.environ.get("GTCRN_LIB_VARIANT")
    if variant in ("stamps", "exp"):     # diagnostic builds: tools/phase_profile.py / tools/ab_bench.py only
        path = LIB_PATH.replace(".so", f"_{variant}.so")
    if not os.path.exists(path):
        raise GtcrnError(
            f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP extension is mandatory, there is no CPU path)")
    # PyTorch ships its own libamdhip64; loading it first makes this library bind to the same runtime
    # (two HIP runtimes in one process: the second one finds no GPU)
    import torch  # noqa: F401
    L = ctypes.CDLL(path)
    ci, cl = ctypes.c_int, ctypes.c_long
    L.gtcrn_abi_version.restype = ci
    L.gtcrn_last_error.restype = ctypes.c_char_p
    L.gtcrn_param_tensors.restype = cl
    L.gtcrn_param_name.restype = ctypes.c_char_p
    L.gtcrn_param_name.argtypes = [cl]
    L.gtcrn_param_numel.restype = cl
    L.gtcrn_param_numel.argtypes = [cl]
    L.gtcrn_param_offset.restype = cl
    L.gtcrn_param_offset.argtypes = [cl]
    L.gtcrn_model_create.argtypes = [ctypes.POINTER(_vp), _c_f32p, cl, ci]
    L.gtcrn_model_set_params.argtypes = [_vp, _c_f32p, cl]
    L.gtcrn_model_destroy.argtypes = [_vp]
    L.gtcrn_model_destroy.restype = None
    L.gtcrn_model_reserve.argtypes = [_vp, ci, ci]
    L.gtcrn_make_window.argtypes = [ci, _c_f32p]
    L.gtcrn_num_frames.restype = cl
    L.gtcrn_num_frames.argtypes = [cl]
    L.gtcrn_stft.argtypes = [_vp, ci, cl, _vp, _vp, cl, cl, cl, _vp]
    L.gtcrn_stft_frames.argtypes = [_vp, ci, cl, _vp, _vp, _vp]
    L.gtcrn_istft.argtypes = [_vp, cl, cl, cl, ci, ci, _vp, _vp, _vp]
    L.gtcrn_forward_spec.argtypes = [_vp, _vp, cl, cl, cl, _vp, cl, cl, cl, ci, ci, _vp]
    L.gtcrn_forward_wave.argtypes = [_vp, _vp, _vp, ci, cl, _vp, _vp]
    L.gtcrn_forward_wave_var.argtypes = [_vp, _vp, _vp, ci, cl, _vp, _vp, _vp]
    cf = ctypes.c_float
    L.gtcrn_forward_spec_quant.argtypes = [_vp, _vp, cl, cl, cl, _vp, cl, cl, cl, ci, ci, cf, cf, _vp]
    L.gtcrn_forward_wave_quant.argtypes = [_vp, _vp, _vp, ci, cl, _vp, cf, cf, _vp]
    L.gtcrn_pack_params_quant_host.argtypes = [_c_f32p, cl, _c_f32p, ctypes.POINTER(ci)]
    L.gtcrn_round_to_half.restype = cf
    L.gtcrn_round_to_half.argtypes = [cf]
    L.gtcrn_stream_state_bytes.restype = ctypes.c_size_t
    L.gtcrn_stream_reset.argtypes = [_vp, _vp, ci, _vp]
    L.gtcrn_stream_step.argtypes = [_vp, _vp, _vp, cl, cl, cl, _vp, cl, cl, cl, ci, ci, _vp]
    L.gtcrn_stream_import.argtypes = [_vp, _vp, ci, _vp, _vp, ctypes.POINTER(_vp), _vp]
    L.gtcrn_stream_export.argtypes = [_vp, _vp, ci, _vp, _vp, ctypes.POINTER(_vp), _vp]
    L.gtcrn_wave_stream_state_bytes.restype = ctypes.c_size_t
    L.gtcrn_wave_stream_reset.argtypes = [_vp, _vp, _vp, ci, _vp]
    for fn in ("gtcrn_wave_stream_step", "gtcrn_wave_stream_step_pcm16"):
        getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, cl, _vp, cl, ci, ci, _vp, _vp]
    for fn in ("gtcrn_wave_stream_flush", "gtcrn_wave_stream_flush_pcm16"):
        getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, cl, ci, _vp, cl, ci, _vp, _vp]
    L.gtcrn_resampler_create.argtypes = [ctypes.POINTER(_vp), ci, ci, ci]
    L.gtcrn_resampler_destroy.argtypes = [_vp]
    L.gtcrn_resampler_destroy.restype = None
    L.gtcrn_resample_taps.restype = cl
    L.gtcrn_resample_taps.argtypes = [ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci), _c_f32p, cl]
    L.gtcrn_resample_out_len.restype = cl
    L.gtcrn_resample_out_len.argtypes = [ci, ci, cl]
    for fn in ("gtcrn_resample", "gtcrn_resample_pcm16_in", "gtcrn_resample_pcm16_out"):
        getattr(L, fn).argtypes = [_vp, _vp, cl, _vp, cl, _vp, cl, ci, _vp]
    L.gtcrn_rate_stream_hop.argtypes = [ci]
    L.gtcrn_rate_stream_latency.argtypes = [ci]
    L.gtcrn_rate_stream_state_bytes.restype = ctypes.c_size_t
    L.gtcrn_rate_stream_state_bytes.argtypes = [ci]
    L.gtcrn_rate_stream_reserve.argtypes = [_vp, _vp, _vp, ci, ci]
    L.gtcrn_rate_stream_reset.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, ci, _vp]
    for fn in ("gtcrn_rate_stream_step", "gtcrn_rate_stream_step_pcm16"):
        getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, cl, _vp, cl, ci, ci, _vp, _vp]
    L.gtcrn_rate_stream_debug_handoff.restype = cl
    L.gtcrn_rate_stream_debug_handoff.argtypes = [_vp, ci, _vp, cl, _vp]
    L.gtcrn_packet_stream_n16.argtypes = [ci, ci]
    L.gtcrn_packet_stream_latency16.argtypes = [ci, ci]
    L.gtcrn_packet_stream_state_bytes.restype = ctypes.c_size_t
    L.gtcrn_packet_stream_state_bytes.argtypes = [ci, ci]
    L.gtcrn_packet_stream_schedule.argtypes = [ci, ci, ci, ctypes.POINTER(ci)]
    L.gtcrn_packet_stream_create.argtypes = [ctypes.POINTER(_vp), _vp, _vp, _vp, ci, ci, ci]
    L.gtcrn_packet_stream_destroy.argtypes = [_vp]
    L.gtcrn_packet_stream_destroy.restype = None
    L.gtcrn_packet_stream_phase.argtypes = [_vp]
    L.gtcrn_packet_stream_next_hops.argtypes = [_vp]
    L.gtcrn_packet_stream_reset.argtypes = [_vp, _vp, _vp, _vp, ci, _vp]
    for fn in ("gtcrn_packet_stream_step", "gtcrn_packet_stream_step_pcm16"):
        getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, _vp, cl, _vp, cl, ci, _vp, _vp]
    L.gtcrn_packet_stream_debug_handoff.restype = cl
    L.gtcrn_packet_stream_debug_handoff.argtypes = [_vp, ci, _vp, cl, _vp]
    # the attenuation-limited forms: the plain argument lists with d_gain in front of d_win
    L.gtcrn_forward_wave_limited.argtypes = [_vp, _vp, _vp, ci, cl, _vp, _vp, _vp, _vp]
    for fn in ("gtcrn_wave_stream_step_limited", "gtcrn_wave_stream_step_limited_pcm16"):
        getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, cl, _vp, cl, ci, ci, _vp, _vp, _vp]
    for fn in ("gtcrn_wave_stream_flush_limited", "gtcrn_wave_stream_flush_limited_pcm16"):
        getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, cl, ci, _vp, cl, ci, _vp, _vp, _vp]
    for fn in ("gtcrn_rate_stream_step_limited", "gtcrn_rate_stream_step_limited_pcm16"):
        getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, cl, _vp, cl, ci, ci, _vp, _vp, _vp]
    L.gtcrn_packet_stream_set_dry_gain.argtypes = [_vp, _vp]
    # stream slots: (model, state[, wstate], slots, count, max_active, ...).  A library of an earlier commit, loaded through
    # LIB_PATH for a same-GPU comparison of the contiguous calls (tools/slot_stream_bench.py --lib), has none of these
    # symbols: it loads, and a slot call on it fails with ctypes' AttributeError at the call.
    if hasattr(L, "gtcrn_stream_step_slots"):
        L.gtcrn_stream_step_slots.argtypes = [_vp, _vp, _vp, _vp, ci, _vp, cl, cl, cl, _vp, cl, cl, cl, _vp]
        L.gtcrn_stream_reset_slots.argtypes = [_vp, _vp, _vp, _vp, _vp, ci, _vp]
        for fn in ("gtcrn_wave_stream_step_slots", "gtcrn_wave_stream_step_slots_pcm16"):
            getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, _vp, ci, _vp, cl, _vp, cl, _vp, _vp, _vp]
        for fn in ("gtcrn_wave_stream_flush_slots", "gtcrn_wave_stream_flush_slots_pcm16"):
            getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, _vp, ci, _vp, cl, ci, _vp, cl, _vp, _vp, _vp]
    # packet stream slots: (handle, state, wstate, pstate, phase, slots, count, max_active, ...)
    if hasattr(L, "gtcrn_packet_stream_step_slots"):
        L.gtcrn_packet_stream_reset_slots.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ci, _vp]
        for fn in ("gtcrn_packet_stream_step_slots", "gtcrn_packet_stream_step_slots_pcm16"):
            getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ci, _vp, cl, _vp, cl, _vp, _vp]
    # level meters (an earlier library has neither symbol: a state with meters then fails at its first step)
    if hasattr(L, "gtcrn_wave_stream_set_meters"):
        L.gtcrn_wave_stream_set_meters.argtypes = [_vp, _vp]
        L.gtcrn_level_dbov.argtypes = [ctypes.c_double, ctypes.c_double]
    # gain ramps (an earlier library has neither symbol: only a state asked for with ramp=True fails, at its creation)
    if hasattr(L, "gtcrn_wave_stream_set_gain_ramp"):
        L.gtcrn_wave_stream_set_gain_ramp.argtypes = [_vp, _vp]
        L.gtcrn_gain_ramp_host.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_float)]
    # level control (an earlier library has none of these: only a state asked for with alc= fails, at its creation)
    if hasattr(L, "gtcrn_wave_stream_set_alc"):
        fp = ctypes.POINTER(ctypes.c_float)
        L.gtcrn_wave_stream_set_alc.argtypes = [_vp, _vp, _vp]
        L.gtcrn_alc_params_host.argtypes = [ctypes.POINTER(AlcConfig), fp]
        L.gtcrn_alc_block_host.argtypes = [fp, fp, fp, fp, fp, fp]
    # tone guard (an earlier library has none of these: only a state asked for with tones= fails, at its creation)
    if hasattr(L, "gtcrn_wave_stream_set_tone"):
        fp = ctypes.POINTER(ctypes.c_float)
        L.gtcrn_wave_stream_set_tone.argtypes = [_vp, _vp, _vp, _vp]
        L.gtcrn_tone_params_host.argtypes = [ctypes.POINTER(ToneConfig), fp]
        L.gtcrn_tone_table_host.argtypes = [fp]
        L.gtcrn_tone_block_host.argtypes = [fp, fp, fp, fp, ctypes.POINTER(ctypes.c_int)]
    # G.711 payloads (an earlier library has none of these: a G.711 state or converter then fails at its first call)
    if hasattr(L, "gtcrn_packet_stream_step_g711"):
        L.gtcrn_packet_stream_step_g711.argtypes = [_vp, _vp, _vp, _vp, _vp, cl, _vp, cl, ci, ci, _vp, _vp]
        L.gtcrn_packet_stream_step_slots_g711.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ci, _vp, cl, _vp, cl, ci, _vp, _vp]
        L.gtcrn_g711_to_f32.argtypes = [ci, ci, _vp, _vp, cl, _vp]
        L.gtcrn_f32_to_g711.argtypes = [ci, ci, _vp, _vp, cl, _vp]
        L.gtcrn_g711_decode_table.argtypes = [ci, ctypes.POINTER(ctypes.c_short)]
        L.gtcrn_g711_encode_pcm16.argtypes = [ci, ci]
    # high band (an earlier library has none of these: a state with highband= then fails at its creation)
    if hasattr(L, "gtcrn_rate_stream_step_hb"):
        L.gtcrn_rate_stream_hb_state_bytes.restype = ctypes.c_size_t
        L.gtcrn_rate_stream_hb_state_bytes.argtypes = [ci]
        L.gtcrn_rate_stream_hb_reset.argtypes = [ci, _vp, ci, _vp]
        for fn in ("gtcrn_rate_stream_step_hb", "gtcrn_rate_stream_step_hb_pcm16"):
            getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, cl, _vp, cl, ci, ci, _vp, _vp, _vp, _vp, _vp]
        L.gtcrn_resample_hb.argtypes = [_vp, _vp, cl, _vp, cl, _vp, cl, _vp, cl, _vp, cl, _vp, _vp, cl, ci, _vp]
    # high band on the packet forms (an earlier library has none of these: a packet state with highband= fails at its creation)
    if hasattr(L, "gtcrn_packet_stream_step_hb"):
        L.gtcrn_packet_stream_hb_latency.argtypes = [ci, ci]
        L.gtcrn_packet_stream_hb_state_bytes.restype = ctypes.c_size_t
        L.gtcrn_packet_stream_hb_state_bytes.argtypes = [ci, ci]
        L.gtcrn_packet_stream_hb_reset.argtypes = [_vp, _vp, ci, _vp]
        L.gtcrn_packet_stream_hb_reset_slots.argtypes = [_vp, _vp, _vp, _vp, ci, _vp]
        for fn in ("gtcrn_packet_stream_step_hb", "gtcrn_packet_stream_step_hb_pcm16"):
            getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, _vp, cl, _vp, cl, ci, _vp, _vp, _vp, _vp]
        for fn in ("gtcrn_packet_stream_step_slots_hb", "gtcrn_packet_stream_step_slots_hb_pcm16"):
            getattr(L, fn).argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ci, _vp, cl, _vp, cl, _vp, _vp, _vp, _vp]
    L.gtcrn_stream_conv2d.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp] + [ci] * 12 + [_vp]
    L.gtcrn_pack_sizes.argtypes = [ctypes.POINTER(cl), ctypes.POINTER(cl)]
    L.gtcrn_pack_sizes.restype = None
    L.gtcrn_pack_params_host.argtypes = [_c_f32p, cl, _c_f32p, ctypes.POINTER(ci)]
    L.gtcrn_debug_enable.argtypes = [_vp, ci]
    L.gtcrn_var_spans_enable.argtypes = [_vp, ci]
    L.gtcrn_stream_form.argtypes = [_vp, ci]
    L.gtcrn_stream_streams_per_workgroup.argtypes = [ci]
    L.gtcrn_debug_tap.restype = cl
    L.gtcrn_debug_tap.argtypes = [_vp, ctypes.c_char_p, ci, _c_f32p, cl]
    L.gtcrn_debug_stamps.restype = cl
    L.gtcrn_debug_stamps.argtypes = [_vp, ci, ctypes.POINTER(ctypes.c_ulonglong), cl]
    L.gtcrn_selftest_mfma.argtypes = [ci]
    L.gtcrn_pcm16_to_f32.argtypes = [ci, _vp, _vp, cl, _vp]
    L.gtcrn_f32_to_pcm16.argtypes = [ci, _vp, _vp, cl, _vp]
    L.gtcrn_selftest_split3.argtypes = [ci, _c_f32p, cl, _c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p]
    L.gtcrn_timing_enable.argtypes = [_vp, ci]
    L.gtcrn_timing_read.argtypes = [_vp, ci, ctypes.c_char_p, ci, _c_f32p, ctypes.POINTER(ci)]
    L.gtcrn_timing_kernels.restype = ci
    L.gtcrn_trainer_create.argtypes = [ctypes.POINTER(_vp), ci]
    L.gtcrn_trainer_destroy.argtypes = [_vp]
    L.gtcrn_trainer_destroy.restype = None
    L.gtcrn_train_workspace_bytes.restype = cl
    L.gtcrn_train_workspace_bytes.argtypes = [ci, ci]
    L.gtcrn_train_workspace_bytes2.restype = cl
    L.gtcrn_train_workspace_bytes2.argtypes = [ci, ci, ci]
    L.gtcrn_trainer_workspace_bytes.restype = cl
    L.gtcrn_trainer_workspace_bytes.argtypes = [_vp, ci, ci]
    L.gtcrn_trainer_set_storage.argtypes = [_vp, ci]
    L.gtcrn_trainer_set_fusions.argtypes = [_vp, ci]
    L.gtcrn_train_forward.argtypes = [_vp, _vp, _vp, cl, cl, cl, _vp, cl, cl, cl, ci, ci, _vp]
    L.gtcrn_train_backward.argtypes = [_vp, _vp, _vp, cl, cl, cl, _vp, cl, cl, cl, _vp, _vp]
    L.gtcrn_train_tap.argtypes = [_vp, ctypes.c_char_p, _vp, ctypes.POINTER(cl), _vp]
    L.gtcrn_train_loss.argtypes = [_vp, _vp, cl, cl, cl, _vp, cl, cl, cl, ci, ci, _vp, _vp, _vp]
    L.gtcrn_train_loss_strided.argtypes = [_vp, _vp, cl, cl, cl, _vp, cl, cl, cl, ci, ci, _vp, _vp, cl, cl, cl, _vp]
    cd = ctypes.c_double
    L.gtcrn_train_loss_terms.argtypes = [_vp, _vp, ci, _vp]
    L.gtcrn_clip_adam_step.argtypes = [ci, _vp, _vp, _vp, _vp, _vp, cl, cf, cd, cd, cd, cd, cd, cl, _vp, _vp, _vp]
    L.gtcrn_clip_adam_workspace_bytes.restype = cl
    L.gtcrn_clip_adam_workspace_bytes.argtypes = [cl]
    L.gtcrn_scorer_create.argtypes = [ctypes.POINTER(_vp), ci]
    L.gtcrn_scorer_destroy.argtypes = [_vp]
    L.gtcrn_scorer_destroy.restype = None
    L.gtcrn_score_workspace_bytes.restype = ctypes.c_size_t
    L.gtcrn_score_workspace_bytes.argtypes = [ci, cl]
    L.gtcrn_score.argtypes = [_vp, _vp, cl, _vp, cl, _vp, cl, ci, ci, _vp, _vp, _vp]
    L.gtcrn_score_taps.restype = cl
    L.gtcrn_score_taps.argtypes = [ctypes.POINTER(ci), ctypes.POINTER(ci), _c_f32p, cl]
    L.gtcrn_score_bands.argtypes = [ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.gtcrn_score_frames.restype = cl
    L.gtcrn_score_frames.argtypes = [cl]
    L.gtcrn_score_debug.restype = cl
    L.gtcrn_score_debug.argtypes = [_vp, ci, ci, _vp, cl, _vp]
    L.gtcrn_score_timing.argtypes = [_vp, ci]
    L.gtcrn_score_timing_read.argtypes = [_vp, ci, ctypes.c_char_p, ci, _c_f32p]
    L.gtcrn_score_ext_workspace_bytes.restype = ctypes.c_size_t
    L.gtcrn_score_ext_workspace_bytes.argtypes = [ci, cl]
    L.gtcrn_score_ext.argtypes = [_vp, _vp, cl, _vp, cl, _vp, cl, ci, ci, _vp, _vp, _vp]
    L.gtcrn_score_segsnr_frames.restype = cl
    L.gtcrn_score_segsnr_frames.argtypes = [cl]
    L.gtcrn_score_segsnr_window.argtypes = [ctypes.POINTER(ctypes.c_double)]
    L.gtcrn_score_ext_stages.argtypes = []
    L.gtcrn_score_ext_timing_read.argtypes = [_vp, ci, ctypes.c_char_p, ci, _c_f32p]
    # training batches from a resident corpus (an earlier library has none of these: data.BatchSource then fails at its creation)
    if hasattr(L, "gtcrn_batch_plan"):
        L.gtcrn_batch_plan.argtypes = [_vp, ci, _vp, ci, ci, cl, cl, ci, cf, cf, cf, cf, _vp, _vp, ci, _vp, _vp]
        L.gtcrn_batch_plan_host.argtypes = [_vp, ci, _vp, ci, ci, cl, cl, ci, cf, cf, cf, cf, _vp, _vp, _vp]
        L.gtcrn_batch_workspace_bytes.restype = ctypes.c_size_t
        L.gtcrn_batch_workspace_bytes.argtypes = [ci, cl]
        L.gtcrn_batch_pairs.argtypes = [_vp, _vp, _vp, ci, _vp, ci, cl, _vp, cl, _vp, cl, _vp]
        L.gtcrn_batch_mix.argtypes = [_vp, _vp, ci, _vp, _vp, ci, _vp, ci, cl, _vp, cl, _vp, cl, _vp, _vp, ci, _vp]
    # reverberant speech for those batches (an earlier library has none of these: data.RirBank then fails at its creation)
    if hasattr(L, "gtcrn_batch_reverb"):
        L.gtcrn_batch_reverb_plan.argtypes = [ci, cf, ci, cl, _vp, _vp, _vp]
        L.gtcrn_batch_reverb_plan_host.argtypes = [ci, cf, ci, cl, _vp, _vp]
        L.gtcrn_batch_reverb_table_bytes.restype = ctypes.c_size_t
        L.gtcrn_batch_reverb_table_bytes.argtypes = [_vp, ci]
        L.gtcrn_batch_reverb_prepare.argtypes = [_vp, _vp, ci, _vp, ctypes.c_size_t, _vp]
        L.gtcrn_batch_reverb_workspace_bytes.restype = ctypes.c_size_t
        L.gtcrn_batch_reverb_workspace_bytes.argtypes = [ci, cl]
        L.gtcrn_batch_reverb.argtypes = [_vp, _vp, ci, _vp, _vp, ci, _vp, ctypes.c_size_t, _vp, _vp, ci, cl, _vp, cl, _vp, _vp,
                                         _vp, _vp, ci, _vp]
        L.gtcrn_selftest_mfma_i8.argtypes = [ci]
    # dereverberation targets: the split convolution and the mix with a target corpus
    if hasattr(L, "gtcrn_batch_reverb_split"):
        L.gtcrn_batch_reverb_split_table_bytes.restype = ctypes.c_size_t
        L.gtcrn_batch_reverb_split_table_bytes.argtypes = [_vp, _vp, ci]
        L.gtcrn_batch_reverb_split_prepare.argtypes = [_vp, _vp, _vp, ci, _vp, ctypes.c_size_t, _vp]
        L.gtcrn_batch_reverb_split_workspace_bytes.restype = ctypes.c_size_t
        L.gtcrn_batch_reverb_split_workspace_bytes.argtypes = [ci, cl]
        L.gtcrn_batch_reverb_split.argtypes = [_vp, _vp, ci, _vp, _vp, _vp, ci, _vp, ctypes.c_size_t, _vp, _vp, ci, cl, _vp, _vp, cl,
                                               _vp, _vp, _vp, _vp, ci, _vp]
        L.gtcrn_batch_mix_target.argtypes = [_vp, _vp, ci, _vp, _vp, ci, _vp, _vp, ci, cl, _vp, cl, _vp, cl, _vp, _vp, ci, _vp]
    # the mix at an SNR of active levels
    if hasattr(L, "gtcrn_batch_mix_active"):
        L.gtcrn_batch_active_workspace_bytes.restype = ctypes.c_size_t
        L.gtcrn_batch_active_workspace_bytes.argtypes = [ci, cl, ci]
        L.gtcrn_batch_mix_active.argtypes = [_vp, _vp, ci, _vp, _vp, ci, _vp, _vp, ci, cl, _vp, cl, _vp, cl, ci, ctypes.c_longlong,
                                             _vp, _vp, ci, _vp]
    # telephone-channel rows: the 8 kHz band and G.711 as a post-pass over drawn rows
    if hasattr(L, "gtcrn_batch_phone"):
        L.gtcrn_batch_phone_taps.argtypes = [_vp]
        L.gtcrn_batch_phone_chunk.argtypes = []
        L.gtcrn_batch_phone_plan.argtypes = [cf, ci, ci, cl, _vp, _vp, _vp]
        L.gtcrn_batch_phone_plan_host.argtypes = [cf, ci, ci, cl, _vp, _vp]
        L.gtcrn_batch_phone.argtypes = [_vp, cl, _vp, cl, _vp, ci, cl, _vp, cl, _vp, cl, ci, _vp, _vp]
        L.gtcrn_batch_phone_host.argtypes = [_vp, cl, _vp, cl, _vp, ci, cl, _vp, cl, _vp, cl, ci, _vp]
    # conference rooms: the mix-minus of the loudest talkers (gtcrn_micro_amd/mixer.py)
    mix_dev = [_vp, cl, ci, _vp, cl, ci, ci, _vp, _vp, ci, ci, _vp, _vp, ci, _vp, _vp, cl, _vp]
    L.gtcrn_mix_params_host.argtypes = [_vp, _vp]
    L.gtcrn_mix_rooms.argtypes = mix_dev
    L.gtcrn_mix_rooms_pcm16.argtypes = mix_dev
    L.gtcrn_mix_rooms_host.argtypes = mix_dev[:-1]
    L.gtcrn_mix_rooms_pcm16_host.argtypes = mix_dev[:-1]
    # packet loss concealment (gtcrn_micro_amd/plc.py)
    plc_dev = [_vp, cl, ci, ci, _vp, _vp, _vp, _vp, cl, _vp, ci, _vp]
    L.gtcrn_plc_params_host.argtypes = [_vp, _vp]
    L.gtcrn_plc_rows.argtypes = plc_dev + [_vp]
    L.gtcrn_plc_rows_pcm16.argtypes = plc_dev + [_vp]
    L.gtcrn_plc_rows_g711.argtypes = plc_dev + [ci, _vp]
    L.gtcrn_plc_reset.argtypes = [_vp, cl, _vp, ci, _vp, _vp, ci, _vp, _vp]
    L.gtcrn_plc_rows_host.argtypes = plc_dev
    L.gtcrn_plc_rows_pcm16_host.argtypes = plc_dev
    L.gtcrn_plc_rows_g711_host.argtypes = plc_dev + [ci]
    if L.gtcrn_abi_version() != 1:
        raise GtcrnError("libgtcrn_micro_hip.so ABI version mismatch")
    _lib = L
    return L


def _check(rc):
    if rc < 0:
        raise GtcrnError(lib().gtcrn_last_error().decode() or f"gtcrn error {rc}")
    return rc


_param_table = None


def param_table():
    """((name, numel, offset), ...) of the canonical blob (reference state_dict order); built once."""
    global _param_table
    if _param_table is None:
        L = lib()
        _param_table = tuple((L.gtcrn_param_name(i).decode(), L.gtcrn_param_numel(i), L.gtcrn_param_offset(i))
                             for i in range(L.gtcrn_param_tensors()))
    return _param_table


def make_window(kind=0):
    w = np.empty(512, np.float32)
    _check(lib().gtcrn_make_window(kind, w.ctypes.data_as(_c_f32p)))
    return w


def num_frames(L):
    return int(lib().gtcrn_num_frames(int(L)))


def pack_params_host(params, quant=False):
    """Host-only: the BN-folded slot-space buffers (floats, ints) the kernels consume; quant=True: with every conv /
    linear weight as fp16(int8 * per-output-channel scale) (the configs[4] variant)."""
    params = np.ascontiguousarray(params, np.float32).ravel()
    nf, ni = ctypes.c_long(), ctypes.c_long()
    lib().gtcrn_pack_sizes(ctypes.byref(nf), ctypes.byref(ni))
    F = np.empty(nf.value, np.float32)
    I = np.empty(ni.value, np.int32)
    fn = lib().gtcrn_pack_params_quant_host if quant else lib().gtcrn_pack_params_host
    _check(fn(params.ctypes.data_as(_c_f32p), params.size, F.ctypes.data_as(_c_f32p),
              I.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    return F, I


def round_to_half(x):
    """float -> IEEE binary16 (round to nearest even) -> float, the host twin of the kernels' v_cvt_f16_f32."""
    return float(lib().gtcrn_round_to_half(float(x)))


def atten_lim_to_gain(db):
    """Attenuation limit in dB -> the dry gain beta = 10^(-db / 20) of the limited calls (include/gtcrn_micro_hip.h,
    "attenuation limit"): None or inf = no limit = 0.0; 0 dB = bypass = 1.0; negative or NaN raises ValueError."""
    if db is None:
        return 0.0
    db = float(db)
    if db != db or db < 0.0:
        raise ValueError(f"the attenuation limit must be >= 0 dB (None or inf: no limit), got {db!r}")
    if db == float("inf"):
        return 0.0
    return float(10.0 ** (-db / 20.0))


def level_dbov(energy, nsamples):
    """RFC 6464 audio level of a window of `nsamples` samples whose squares sum to `energy` (full scale 1.0): -dBov rounded
    to the nearest integer, 0 (loudest) .. 127 (silence, also for energy <= 0 or nsamples <= 0).  gtcrn_level_dbov, on the
    host; scalars give an int, arrays (broadcast against each other) an int32 array."""
    fn = lib().gtcrn_level_dbov
    if np.ndim(energy) == 0 and np.ndim(nsamples) == 0:
        return int(fn(float(energy), float(nsamples)))
    e, n = np.broadcast_arrays(np.asarray(energy, np.float64), np.asarray(nsamples, np.float64))
    return np.array([fn(float(a), float(b)) for a, b in zip(e.ravel(), n.ravel())], np.int32).reshape(e.shape)


def gain_ramp(p, g):
    """The 256 dry gains of a block that ramps from `p`, where the stream's last block ended, to `g` (include/
    gtcrn_micro_hip.h, "gain ramps"): a float32 array from gtcrn_gain_ramp_host, the function the kernel compiles, on the
    host."""
    fn = getattr(lib(), "gtcrn_gain_ramp_host", None)
    if fn is None:
        raise GtcrnError("this library has no gain ramps")
    out = np.empty(256, np.float32)
    _check(fn(float(np.float32(p)), float(np.float32(g)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return out


class AlcConfig(ctypes.Structure):
    """gtcrn_alc_config of include/gtcrn_micro_hip.h, "level control"."""
    _fields_ = [(k, ctypes.c_double) for k in ("target_dbov", "min_gain_db", "max_gain_db", "rise_db_s", "fall_db_s",
                                               "ceiling_dbov", "floor_dbov", "ratio_db", "hang_ms", "alpha")] + [("mode", ctypes.c_int)]


ALC_DEFAULTS = dict(target_dbov=-26.0, min_gain_db=-6.0, max_gain_db=24.0, rise_db_s=6.0, fall_db_s=30.0, ceiling_dbov=-1.0,
                    floor_dbov=-45.0, ratio_db=-10.0, hang_ms=200.0, alpha=0.0625, mode=1)     # GTCRN_ALC_DEFAULTS


def _alc_fields(alc):
    """alc= of the state constructors -> the config's fields: "vad" (measure only), True (the defaults) or a mapping."""
    if isinstance(alc, str):
        if alc != "vad":
            raise GtcrnError(f'alc must be None, "vad", True or a mapping of the config\'s fields, got {alc!r}')
        return dict(ALC_DEFAULTS, mode=0)
    if alc is True:
        return dict(ALC_DEFAULTS)
    if not hasattr(alc, "keys"):
        raise GtcrnError(f'alc must be None, "vad", True or a mapping of the config\'s fields, got {alc!r}')
    return dict(ALC_DEFAULTS, **{str(k): alc[k] for k in alc.keys()})


def alc_params(**fields):
    """The 16 parameter words of the level control (include/gtcrn_micro_hip.h, "level control") for the defaults with
    `fields` replaced: a float32 array from gtcrn_alc_params_host, the one place the words are made."""
    fn = getattr(lib(), "gtcrn_alc_params_host", None)
    if fn is None:
        raise GtcrnError("this library has no level control")
    unknown = set(fields) - set(ALC_DEFAULTS)
    if unknown:
        raise GtcrnError(f"unknown level-control fields {sorted(unknown)}: the config has {sorted(ALC_DEFAULTS)}")
    f = dict(ALC_DEFAULTS, **fields)
    cfg = AlcConfig(*[float(f[k]) for k, _ in AlcConfig._fields_[:-1]], int(f["mode"]))
    out = np.empty(16, np.float32)
    _check(fn(ctypes.byref(cfg), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return out


def alc_block(params, record, w, x, m):
    """One emitted block through gtcrn_alc_block_host, the functions the kernel compiles, on the host: the 16 parameter
    words, the stream's 8-word record and the 256-sample blocks w (wet), x (dry) and m (what the call would store) ->
    (y, the record after the block), both float32 arrays.  The structural zero of a stream's first block is the caller's."""
    fn = getattr(lib(), "gtcrn_alc_block_host", None)
    if fn is None:
        raise GtcrnError("this library has no level control")
    arr = [np.ascontiguousarray(v, np.float32) for v in (params, record, w, x, m)]
    if [v.shape for v in arr] != [(16,), (8,), (256,), (256,), (256,)]:
        raise GtcrnError("alc_block takes 16 parameter words, an 8-word record and three blocks of 256 samples")
    rec, y = arr[1].copy(), np.empty(256, np.float32)
    ptr = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    _check(fn(ptr(arr[0]), ptr(rec), ptr(arr[2]), ptr(arr[3]), ptr(arr[4]), ptr(y)))
    return y, rec


def _alc_on(alc):
    """alc= of the state constructors: None and False are off, like meters=False and ramp=False."""
    return alc is not None and alc is not False


def _alc_without_highband(alc, highband):
    if _alc_on(alc) and highband is not None:
        raise GtcrnError("alc= and highband= do not go together: the high band's formulas assume the 16 kHz hand-off at unit gain")


class ToneConfig(ctypes.Structure):
    """gtcrn_tone_config of include/gtcrn_micro_hip.h, "tone guard"."""
    _fields_ = [(k, ctypes.c_double) for k in ("min_dbov", "twist_db", "dominance_db", "pair_purity", "single_purity")] + \
               [(k, ctypes.c_int) for k in ("guard_blocks", "digit_blocks", "single_blocks", "hold_blocks", "mode", "singles")]


TONE_DEFAULTS = dict(min_dbov=-45.0, twist_db=8.0, dominance_db=8.0, pair_purity=0.6, single_purity=0.8, guard_blocks=1,
                     digit_blocks=2, single_blocks=4, hold_blocks=1, mode=1, singles=1)     # GTCRN_TONE_DEFAULTS
TONE_FREQS = (697, 770, 852, 941, 1209, 1336, 1477, 1633, 1100, 2100)


def _tone_fields(tones):
    """tones= of the state constructors -> the config's fields: "detect" (no guard), True (the defaults) or a mapping."""
    if isinstance(tones, str):
        if tones != "detect":
            raise GtcrnError(f'tones must be None, "detect", True or a mapping of the config\'s fields, got {tones!r}')
        return dict(TONE_DEFAULTS, mode=0)
    if tones is True:
        return dict(TONE_DEFAULTS)
    if not hasattr(tones, "keys"):
        raise GtcrnError(f'tones must be None, "detect", True or a mapping of the config\'s fields, got {tones!r}')
    return dict(TONE_DEFAULTS, **{str(k): tones[k] for k in tones.keys()})


def tone_params(**fields):
    """The 16 parameter words of the tone guard (include/gtcrn_micro_hip.h, "tone guard") for the defaults with `fields`
    replaced: a float32 array from gtcrn_tone_params_host, the one place the words are made."""
    fn = getattr(lib(), "gtcrn_tone_params_host", None)
    if fn is None:
        raise GtcrnError("this library has no tone guard")
    unknown = set(fields) - set(TONE_DEFAULTS)
    if unknown:
        raise GtcrnError(f"unknown tone-guard fields {sorted(unknown)}: the config has {sorted(TONE_DEFAULTS)}")
    f = dict(TONE_DEFAULTS, **fields)
    ints = [f[k] for k, t in ToneConfig._fields_ if t is ctypes.c_int]
    if any(int(v) != v for v in ints):
        raise GtcrnError("the tone guard's counts, mode and singles are integers")
    cfg = ToneConfig(*[float(f[k]) for k, t in ToneConfig._fields_ if t is ctypes.c_double], *[int(v) for v in ints])
    out = np.empty(16, np.float32)
    _check(fn(ctypes.byref(cfg), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return out


def tone_table():
    """The tone guard's table from gtcrn_tone_table_host: (10, 256, 2) float32, [f, i] = {cos, sin}(2 pi F_f i / 16000)."""
    fn = getattr(lib(), "gtcrn_tone_table_host", None)
    if fn is None:
        raise GtcrnError("this library has no tone guard")
    out = np.empty((10, 256, 2), np.float32)
    _check(fn(out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return out


def tone_block(params, table, record, x):
    """Steps 1 and 3..5 of one emitted block through gtcrn_tone_block_host, the functions the kernel compiles, on the host:
    the 16 parameter words, the table, the stream's 8-word record and the 256 dry samples -> (the record after the block,
    whether the block is passed dry).  The structural zero of a stream's first block and step 7's counts are the caller's."""
    fn = getattr(lib(), "gtcrn_tone_block_host", None)
    if fn is None:
        raise GtcrnError("this library has no tone guard")
    arr = [np.ascontiguousarray(v, np.float32) for v in (params, table, record, x)]
    if [v.size for v in arr] != [16, 5120, 8, 256]:
        raise GtcrnError("tone_block takes 16 parameter words, the 10 x 256 x 2 table, an 8-word record and 256 samples")
    rec, guard = arr[2].reshape(8).copy(), ctypes.c_int(0)
    ptr = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    _check(fn(ptr(arr[0]), ptr(arr[1]), ptr(rec), ptr(arr[3]), ctypes.byref(guard)))
    return rec, bool(guard.value)


def _tones_on(tones):
    """tones= of the state constructors: None and False are off."""
    return tones is not None and tones is not False


def _attach_live(st, atten_lim_db, meters, ramp, alc, tones=None):
    """The options of a fresh state behind its reset, in this order: the limit, the meter records (True: new zeroed ones;
    else the records, or None, of the wave state it was made from), the ramp words, the level control and the tone guard."""
    import torch
    if atten_lim_db is not None:
        st.set_atten_lim_db(atten_lim_db)
    st.meters = torch.zeros((st.n, 4), device=st.window.device, dtype=torch.float32) if meters is True else meters
    if ramp:
        st._new_gain_ramp()
    if _alc_on(alc):
        st._new_alc(alc)
    if _tones_on(tones):
        st._new_tones(tones)
    return st


def _stream_range(n, lo, hi):
    """lo, hi (None: n) of a call on streams lo..hi-1 of n, as ints."""
    hi = n if hi is None else int(hi)
    lo = int(lo)
    if not 0 <= lo < hi <= n:
        raise GtcrnError(f"stream range [{lo}, {hi}) outside [0, {n})")
    return lo, hi


def _entry(name, x):
    """The entry point `name` for float32 rows x, its _pcm16 twin for int16 ones."""
    import torch
    return getattr(lib(), name + "_pcm16" if x.dtype == torch.int16 else name)


def _gains_of(db, n):
    """db: None, a number, or a sequence of n of them -> a float (one gain for all) or a float32 array of n gains."""
    if db is None or np.isscalar(db):
        return atten_lim_to_gain(db)
    seq = list(db)
    if len(seq) != n:
        raise GtcrnError(f"expected one attenuation limit or {n} of them, got {len(seq)}")
    return np.asarray([atten_lim_to_gain(v) for v in seq], np.float32)


def _stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _spec_strides(t):
    """(sb, sf, st) in elements of a (B,257,T,2) float32 tensor whose last dim is contiguous."""
    assert t.dim() == 4 and t.shape[1] == NBINS and t.shape[3] == 2
    if t.stride(3) != 1:
        raise GtcrnError("the re/im pair of a spectrogram must be contiguous")
    return t.stride(0), t.stride(1), t.stride(2)


def empty_spec(B, T, device, frame_major=False):
    """An uninitialised (B,257,T,2) float32 spectrogram.  frame_major: the memory is (B,T,257,2) -- a frame's 257 bins are
    one 2 KB row, which is how every kernel of this library walks a spectrogram -- viewed in the reference's shape."""
    import torch
    if frame_major:
        return torch.empty((B, T, NBINS, 2), device=device, dtype=torch.float32).permute(0, 2, 1, 3)
    return torch.empty((B, NBINS, T, 2), device=device, dtype=torch.float32)


def _empty_spec_like(t):
    """A new spectrogram with the shape of t and t's memory order (frame-major stays frame-major)."""
    B, _, T, _ = t.shape
    return empty_spec(B, T, t.device, frame_major=abs(t.stride(2)) > abs(t.stride(1)))


def _require_cuda_f32(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise GtcrnError(f"{what} must be a CUDA (ROCm) tensor: this implementation has no CPU path")
    if t.dtype != torch.float32:
        raise GtcrnError(f"{what} must be float32")


def stft(wave, window, out=None, frame_major=False):
    """torch.stft(x,512,256,512,window,return_complex=False) on the GPU: (B,L) or (L,) -> (B,257,T,2)/(257,T,2).
    frame_major: see empty_spec (same shape and values, the library's preferred memory order)."""
    import torch
    _require_cuda_f32(wave, "wave")
    squeeze = wave.dim() == 1
    w2 = wave.reshape(1, -1) if squeeze else wave
    w2 = w2.contiguous()
    B, L = w2.shape
    if L < 257:
        raise GtcrnError("reflect padding needs more than 256 samples")
    T = num_frames(L)
    win = window.to(device=wave.device, dtype=torch.float32).contiguous()
    spec = out if out is not None else empty_spec(B, T, wave.device, frame_major)
    sb, sf, st = _spec_strides(spec)
    with torch.cuda.device(wave.device):
        _check(lib().gtcrn_stft(w2.data_ptr(), B, L, win.data_ptr(), spec.data_ptr(), sb, sf, st, _stream_ptr()))
    return spec[0] if squeeze else spec


def stft_frames(wave, window):
    import torch
    _require_cuda_f32(wave, "wave")
    w2 = (wave.reshape(1, -1) if wave.dim() == 1 else wave).contiguous()
    B, L = w2.shape
    T = num_frames(L)
    win = window.to(device=wave.device, dtype=torch.float32).contiguous()
    fr = torch.empty((B, T, 512), device=wave.device, dtype=torch.float32)
    with torch.cuda.device(wave.device):
        _check(lib().gtcrn_stft_frames(w2.data_ptr(), B, L, win.data_ptr(), fr.data_ptr(), _stream_ptr()))
    return fr


def istft(spec, window):
    """torch.istft(view_as_complex(spec),512,256,512,window): (B,257,T,2)/(257,T,2) -> (B,256(T-1))/(256(T-1),)."""
    import torch
    _require_cuda_f32(spec, "spec")
    squeeze = spec.dim() == 3
    s4 = spec.unsqueeze(0) if squeeze else spec
    if s4.stride(3) != 1:
        s4 = s4.contiguous()
    B, _, T, _ = s4.shape
    if T < 2:
        raise GtcrnError("iSTFT needs at least 2 frames")
    win = window.to(device=spec.device, dtype=torch.float32).contiguous()
    out = torch.empty((B, 256 * (T - 1)), device=spec.device, dtype=torch.float32)
    sb, sf, st = _spec_strides(s4)
    with torch.cuda.device(spec.device):
        _check(lib().gtcrn_istft(s4.data_ptr(), sb, sf, st, B, T, win.data_ptr(), out.data_ptr(), _stream_ptr()))
    return out[0] if squeeze else out


def stream_conv2d(x, cache, weight, bias, kt, kf, dt=1, df=1, pad_f=0, groups=1, transposed=False):
    """Causal streaming conv step on the GPU (see gtcrn_stream_conv2d): returns (y, new_cache)."""
    import torch
    _require_cuda_f32(x, "x")
    x = x.contiguous()
    B, Cin, T, F = x.shape
    Cout = weight.shape[1] if transposed else weight.shape[0]
    H = (kt - 1) * dt
    if cache is None:
        cache = torch.zeros((B, Cin, H, F), device=x.device, dtype=torch.float32)
    cache = cache.contiguous()
    Fout = F - 2 * pad_f + df * (kf - 1) if transposed else F + 2 * pad_f - df * (kf - 1)
    y = torch.empty((B, Cout, T, Fout), device=x.device, dtype=torch.float32)
    new_cache = torch.empty_like(cache)
    w = weight.detach().to(device=x.device, dtype=torch.float32).contiguous()
    bptr = bias.detach().to(device=x.device, dtype=torch.float32).contiguous() if bias is not None else None
    with torch.cuda.device(x.device):
        rc = lib().gtcrn_stream_conv2d(x.data_ptr(), cache.data_ptr(), w.data_ptr(),
                                       bptr.data_ptr() if bptr is not None else None, y.data_ptr(),
                                       new_cache.data_ptr(), B, Cin, Cout, T, F, kt, kf, dt, df, pad_f, groups,
                                       int(bool(transposed)), _stream_ptr())
    _check(rc)
    assert rc == Fout
    return y, new_cache


class Engine:
    """One model handle (gtcrn_model) on one device."""

    def __init__(self, params, device=0):
        params = np.ascontiguousarray(params, np.float32).ravel()
        if params.size != NPARAM_FLOATS:
            raise GtcrnError(f"parameter blob must hold {NPARAM_FLOATS} floats, got {params.size}")
        self.device = int(device)
        h = ctypes.c_void_p()
        _check(lib().gtcrn_model_create(ctypes.byref(h), params.ctypes.data_as(_c_f32p), params.size, self.device))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().gtcrn_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params):
        params = np.ascontiguousarray(params, np.float32).ravel()
        _check(lib().gtcrn_model_set_params(self._h, params.ctypes.data_as(_c_f32p), params.size))

    def reserve(self, B, T):
        _check(lib().gtcrn_model_reserve(self._h, int(B), int(T)))

    def _dev(self):
        import torch
        return torch.cuda.device(self.device)

    def forward_spec(self, spec, out=None):
        import torch
        _require_cuda_f32(spec, "spec")
        if spec.dim() != 4 or spec.shape[1] != NBINS or spec.shape[3] != 2:
            raise GtcrnError(f"spec must be (B,257,T,2), got {tuple(spec.shape)}")
        if spec.device.index != self.device:
            raise GtcrnError("spec is on a different device than the model")
        if spec.stride(3) != 1:
            spec = spec.contiguous()
        B, _, T, _ = spec.shape
        if out is None:
            out = torch.empty((B, NBINS, T, 2), device=spec.device, dtype=torch.float32)
        else:
            self._check_on_device(out, "out")
            if tuple(out.shape) != (B, NBINS, T, 2) or out.stride(3) != 1:
                raise GtcrnError(f"out must be (B,257,{T},2) with contiguous re/im pairs, got {tuple(out.shape)}")
        isb, isf, ist = _spec_strides(spec)
        osb, osf, ost = _spec_strides(out)
        with self._dev():
            _check(lib().gtcrn_forward_spec(self._h, spec.data_ptr(), isb, isf, ist, out.data_ptr(), osb, osf, ost,
                                            B, T, _stream_ptr()))
        return out

    def _check_on_device(self, t, what, shape=None):
        import torch
        _require_cuda_f32(t, what)
        if t.device.index != self.device:
            raise GtcrnError(f"{what} is on cuda:{t.device.index}, the model on cuda:{self.device}")
        if shape is not None and (tuple(t.shape) != tuple(shape) or not t.is_contiguous()):
            raise GtcrnError(f"{what} must be a contiguous float32 tensor of shape {tuple(shape)}, got "
                             f"{tuple(t.shape)} (contiguous: {t.is_contiguous()})")

    def _dry_gain(self, dry_gain, B, device):
        """None, a float in [0, 1] or a (B,) float32 CUDA tensor of them -> None or the (B,) device tensor.  The kernels
        take 0 <= beta <= 1 as a precondition; it is checked here (a tensor's check reads it back: one synchronisation)."""
        import torch
        if dry_gain is None:
            return None
        if isinstance(dry_gain, torch.Tensor):
            g = dry_gain
            if not g.is_cuda or g.dtype != torch.float32 or g.device != device or tuple(g.shape) != (B,) or not g.is_contiguous():
                raise GtcrnError(f"dry_gain must be a float or a contiguous ({B},) float32 tensor on {device}, got "
                                 f"{tuple(g.shape)} {g.dtype} on {g.device}")
            lo, hi = (float(v) for v in torch.aminmax(g))
            if not (0.0 <= lo and hi <= 1.0):
                raise GtcrnError(f"every dry gain must lie in [0, 1], got min {lo} max {hi}")
            return g
        v = float(dry_gain)
        if not 0.0 <= v <= 1.0:
            raise GtcrnError(f"the dry gain must lie in [0, 1], got {v!r}")
        return torch.full((B,), v, device=device, dtype=torch.float32)

    def forward_wave(self, wave, window, out=None, dry_gain=None):
        """dry_gain (None, a float or a (B,) CUDA float tensor, each in [0, 1]): the attenuation limit, beta =
        atten_lim_to_gain(dB); row b becomes fl(fl(beta_b x) + fl(fl(1 - beta_b) y)), x the input cut to the output's
        length (gtcrn_forward_wave_limited).  None: the plain call."""
        import torch
        self._check_on_device(wave, "wave")
        w2 = (wave.reshape(1, -1) if wave.dim() == 1 else wave).contiguous()
        if w2.dim() != 2:
            raise GtcrnError(f"wave must be (B,L) or (L,), got {tuple(wave.shape)}")
        B, L = w2.shape
        T = num_frames(L)
        win = window.to(device=wave.device, dtype=torch.float32).contiguous()
        if out is None:
            out = torch.empty((B, 256 * (T - 1)), device=wave.device, dtype=torch.float32)
        else:
            self._check_on_device(out, "out", (B, 256 * (T - 1)))
        gain = self._dry_gain(dry_gain, B, w2.device)
        with self._dev():
            if gain is None:
                _check(lib().gtcrn_forward_wave(self._h, w2.data_ptr(), out.data_ptr(), B, L, win.data_ptr(),
                                                _stream_ptr()))
            else:
                _check(lib().gtcrn_forward_wave_limited(self._h, w2.data_ptr(), out.data_ptr(), B, L, None, gain.data_ptr(),
                                                        win.data_ptr(), _stream_ptr()))
        return out[0] if wave.dim() == 1 else out

    # ---- int8-weight / fp16-activation variant (BASELINE configs[4]; contract in include/gtcrn_micro_hip.h) ------
    def forward_spec_quant(self, spec, in_scale=0.0, out_scale=0.0, out=None):
        import torch
        self._check_on_device(spec, "spec")
        if spec.dim() != 4 or spec.shape[1] != NBINS or spec.shape[3] != 2:
            raise GtcrnError(f"spec must be (B,257,T,2), got {tuple(spec.shape)}")
        if spec.stride(3) != 1:
            spec = spec.contiguous()
        B, _, T, _ = spec.shape
        if out is None:
            out = torch.empty((B, NBINS, T, 2), device=spec.device, dtype=torch.float32)
        else:
            self._check_on_device(out, "out")
            if tuple(out.shape) != (B, NBINS, T, 2) or out.stride(3) != 1:
                raise GtcrnError(f"out must be (B,257,{T},2) with contiguous re/im pairs, got {tuple(out.shape)}")
        isb, isf, ist = _spec_strides(spec)
        osb, osf, ost = _spec_strides(out)
        with self._dev():
            _check(lib().gtcrn_forward_spec_quant(self._h, spec.data_ptr(), isb, isf, ist, out.data_ptr(), osb, osf,
                                                  ost, B, T, float(in_scale), float(out_scale), _stream_ptr()))
        return out

    def forward_wave_quant(self, wave, window, in_scale=0.0, out_scale=0.0, out=None):
        import torch
        self._check_on_device(wave, "wave")
        w2 = (wave.reshape(1, -1) if wave.dim() == 1 else wave).contiguous()
        if w2.dim() != 2:
            raise GtcrnError(f"wave must be (B,L) or (L,), got {tuple(wave.shape)}")
        B, L = w2.shape
        T = num_frames(L)
        win = window.to(device=wave.device, dtype=torch.float32).contiguous()
        if out is None:
            out = torch.empty((B, 256 * (T - 1)), device=wave.device, dtype=torch.float32)
        else:
            self._check_on_device(out, "out", (B, 256 * (T - 1)))
        with self._dev():
            _check(lib().gtcrn_forward_wave_quant(self._h, w2.data_ptr(), out.data_ptr(), B, L, win.data_ptr(),
                                                  float(in_scale), float(out_scale), _stream_ptr()))
        return out[0] if wave.dim() == 1 else out

    def forward_wave_var(self, wave, lengths, window, out=None, dry_gain=None):
        """Clips of different lengths through ONE launch sequence: ``wave`` (B,Lmax) holds clip b in its first
        ``lengths[b]`` samples (257 <= lengths[b] <= Lmax).  Returns (B, 256*(Lmax//256)); row b carries its
        256*(lengths[b]//256) enhanced samples (bit-identical to forward_wave on that clip alone), the rest of the
        row is unspecified (not written).  dry_gain: as in forward_wave, one gain per clip."""
        import torch
        self._check_on_device(wave, "wave")
        if wave.dim() != 2 or not wave.is_contiguous():
            raise GtcrnError("wave must be a contiguous (B,Lmax) tensor")
        B, L = wave.shape
        lens = torch.as_tensor(lengths, dtype=torch.int32).reshape(-1)
        if lens.numel() != B:
            raise GtcrnError(f"lengths must hold {B} entries, got {lens.numel()}")
        lmin, lmax = int(lens.min()), int(lens.max())
        if lmin < 257 or lmax > L:
            raise GtcrnError(f"every length must lie in [257, Lmax={L}], got min {lmin} max {lmax}")
        lens = lens.to(wave.device)
        T = num_frames(L)
        win = window.to(device=wave.device, dtype=torch.float32).contiguous()
        if out is None:
            out = torch.empty((B, 256 * (T - 1)), device=wave.device, dtype=torch.float32)
        else:
            self._check_on_device(out, "out", (B, 256 * (T - 1)))
        gain = self._dry_gain(dry_gain, B, wave.device)
        with self._dev():
            if gain is None:
                _check(lib().gtcrn_forward_wave_var(self._h, wave.data_ptr(), out.data_ptr(), B, L, lens.data_ptr(),
                                                    win.data_ptr(), _stream_ptr()))
            else:
                _check(lib().gtcrn_forward_wave_limited(self._h, wave.data_ptr(), out.data_ptr(), B, L, lens.data_ptr(),
                                                        gain.data_ptr(), win.data_ptr(), _stream_ptr()))
        return out

    # ---- streaming -----------------------------------------------------------------------
    @staticmethod
    def state_bytes():
        return int(lib().gtcrn_stream_state_bytes())

    def new_state(self, nstreams):
        import torch
        st = torch.empty((nstreams, self.state_bytes() // 4), device=f"cuda:{self.device}", dtype=torch.float32)
        self.stream_reset(st)
        return st

    def stream_reset(self, state, lo=0, hi=None):
        """Resets streams lo..hi-1 of a state of new_state to the start of a new clip (gtcrn_stream_reset on those rows)."""
        self._check_on_device(state, "state")
        if state.dim() != 2 or state.shape[1] != self.state_bytes() // 4 or not state.is_contiguous():
            raise GtcrnError(f"state must be a contiguous (N, {self.state_bytes() // 4}) tensor of new_state")
        lo, hi = _stream_range(state.shape[0], lo, hi)
        with self._dev():
            _check(lib().gtcrn_stream_reset(self._h, state[lo:hi].data_ptr(), hi - lo, _stream_ptr()))

    def stream_step(self, state, spec_t, out=None):
        import torch
        self._check_on_device(spec_t, "spec")
        if spec_t.dim() != 4 or spec_t.shape[1] != NBINS or spec_t.shape[3] != 2:
            raise GtcrnError(f"spec must be (N,257,n,2), got {tuple(spec_t.shape)}")
        if spec_t.stride(3) != 1:
            spec_t = spec_t.contiguous()
        N, _, nfr, _ = spec_t.shape
        self._check_on_device(state, "state", (N, self.state_bytes() // 4))
        if out is None:
            out = torch.empty((N, NBINS, nfr, 2), device=spec_t.device, dtype=torch.float32)
        else:
            self._check_on_device(out, "out")
            if tuple(out.shape) != (N, NBINS, nfr, 2) or out.stride(3) != 1:
                raise GtcrnError(f"out must be (N,257,{nfr},2) with contiguous re/im pairs, got {tuple(out.shape)}")
        isb, isf, ist = _spec_strides(spec_t)
        osb, osf, ost = _spec_strides(out)
        with self._dev():
            _check(lib().gtcrn_stream_step(self._h, state.data_ptr(), spec_t.data_ptr(), isb, isf, ist,
                                           out.data_ptr(), osb, osf, ost, N, nfr, _stream_ptr()))
        return out

    # ---- hop-level waveform streaming (contract: include/gtcrn_micro_hip.h, gtcrn_wave_stream_*) ----------------
    @staticmethod
    def wave_state_bytes():
        return int(lib().gtcrn_wave_stream_state_bytes())

    def new_wave_state(self, nstreams, window, atten_lim_db=None, meters=False, ramp=False, alc=None, tones=None):
        """State of `nstreams` waveform streams: the model state, the wave state (input ring, overlap-add tail, hop
        counter) and the analysis / synthesis window, checked here once: 512 floats with window[0] == 0 (which the
        one-hop-delay contract rests on; torch.hann_window(512).pow(0.5) of infer.py:65 has it).  atten_lim_db (a
        number or one per stream; None: off): the attenuation limit, kept as the per-stream gains ``state.dry_gain``
        that every step and flush of the state then applies (WaveStreamState.set_atten_lim_db rewrites them).
        meters=True: the state owns ``state.meters``, (n, 4) float32 records {E_dry, E_out, peak, blocks} per stream (the
        header's "level meters"), zeroed here, which every step and flush through the state then updates on the device
        (WaveStreamState.reset_meters starts a new window, .levels() reads the RFC 6464 levels).
        ramp=True: the state owns ``state.gain_ramp``, (n,) float32, the gain each stream's last block ended at (the header's
        "gain ramps"): a later change of the limit is then spread over the next emitted block instead of landing as a
        step.  It starts equal to ``state.dry_gain``, which is allocated (zeros: no limit) when atten_lim_db is None.
        alc ("vad": measure only; True: the defaults; a mapping of gtcrn_alc_config's fields; None or False: off): the header's "level
        control" -- the state owns ``state.alc``, (n, 8) float32 records {a, S, hang, voice, voiced, blocks, 0, 0}, and
        ``state.alc_params``, (16,) float32, which every step and flush through the state then uses (WaveStreamState.voice,
        .alc_gain_db, .set_alc, .reset_alc).
        tones ("detect": detect only; True: the defaults; a mapping of gtcrn_tone_config's fields; None or False: off): the
        header's "tone guard" -- the state owns ``state.tones``, (n, 8) float32 records {tone, cand, run, hold, guard, events,
        guarded, blocks}, ``state.tone_params``, (16,) float32, and ``state.tone_table``; every step and flush through the state
        then detects DTMF / 1100 Hz / 2100 Hz per stream and (unless "detect") passes the blocks that hold one dry
        (WaveStreamState.tone, .tone_events, .set_tones, .reset_tones)."""
        import torch
        n = int(nstreams)
        if n < 1:
            raise GtcrnError("nstreams must be >= 1")
        if not isinstance(window, torch.Tensor):
            window = torch.as_tensor(np.asarray(window, np.float32))
        win = window.detach().to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        if win.dim() != 1 or win.numel() != 512:
            raise GtcrnError(f"the window must hold 512 samples, got shape {tuple(window.shape)}")
        if float(win[0]) != 0.0:
            raise GtcrnError(f"the window must have window[0] == 0 (periodic Hann-type), got {float(win[0])!r}")
        st = WaveStreamState(self.new_state(n),
                             torch.empty((n, self.wave_state_bytes() // 4), device=win.device, dtype=torch.float32), win)
        self.wave_stream_reset(st)
        return _attach_live(st, atten_lim_db, True if meters else None, ramp, alc, tones)

    def _bind_live(self, state):
        """Ahead of every step or flush through a state: its meters, ramp words and level control go to the model."""
        self._set_meters(state)
        self._set_gain_ramp(state)
        self._set_alc(state)
        self._set_tones(state)

    def _set_tones(self, state):
        """Hands the state's tone records, parameter words and table to the model ahead of a step or flush, or clears the
        model's pointers for a state without: two states on one engine do not leak into each other."""
        fn = getattr(lib(), "gtcrn_wave_stream_set_tone", None)
        if fn is None:
            return                                       # (an earlier library: _new_tones refused, nothing to clear)
        if state.tones is None:
            _check(fn(self._h, None, None, None))
        else:
            _check(fn(self._h, state.tones.data_ptr(), state.tone_params.data_ptr(), state.tone_table.data_ptr()))

    def _set_alc(self, state):
        """Hands the state's level-control records and parameter words to the model ahead of a step or flush, or clears
        the model's pointers for a state without: two states on one engine do not leak into each other."""
        fn = getattr(lib(), "gtcrn_wave_stream_set_alc", None)
        if fn is None:
            return                                       # (an earlier library: _new_alc refused, nothing to clear)
        if state.alc is None:
            _check(fn(self._h, None, None))
        else:
            _check(fn(self._h, state.alc.data_ptr(), state.alc_params.data_ptr()))

    def _set_gain_ramp(self, state):
        """Hands the state's ramp words to the model ahead of a step or flush, or clears the model's pointer for a state
        without ramps: two states on one engine do not leak into each other."""
        fn = getattr(lib(), "gtcrn_wave_stream_set_gain_ramp", None)
        if fn is None:
            return                                       # (an earlier library: _new_gain_ramp refused, nothing to clear)
        _check(fn(self._h, None if state.gain_ramp is None else state.gain_ramp.data_ptr()))

    def _set_meters(self, state):
        """Hands the state's records to the model ahead of a step or flush, or clears the model's pointer for a state
        without meters: two states on one engine do not leak into each other."""
        fn = getattr(lib(), "gtcrn_wave_stream_set_meters", None)
        if fn is None and state.meters is None:
            return                                       # (an earlier library, loaded for a comparison: nothing to clear)
        if fn is None:
            raise GtcrnError("this library has no level meters")
        _check(fn(self._h, None if state.meters is None else state.meters.data_ptr()))

    def wave_stream_reset(self, state, lo=0, hi=None):
        """Resets streams lo..hi-1 (both states) to the start of a new clip."""
        lo, hi = _stream_range(state.n, lo, hi)
        with self._dev():
            _check(lib().gtcrn_wave_stream_reset(self._h, state.model[lo:hi].data_ptr(), state.wave[lo:hi].data_ptr(),
                                                 hi - lo, _stream_ptr()))

    def _wave_rows(self, state, x, what, g711=False):
        import torch
        kinds = (torch.float32, torch.int16, torch.uint8) if g711 else (torch.float32, torch.int16)   # (uint8: the packet forms)
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in kinds:
            raise GtcrnError(f"{what} must be a float32 or int16 CUDA (ROCm) tensor")
        if x.device.index != self.device:
            raise GtcrnError(f"{what} is on cuda:{x.device.index}, the model on cuda:{self.device}")
        if not isinstance(state, WaveStreamState) or state.model.device != x.device:
            raise GtcrnError("state must come from new_wave_state on the model's device")
        if x.dim() != 2 or x.shape[0] != state.n:
            raise GtcrnError(f"{what} must be ({state.n}, samples), got {tuple(x.shape)}")
        if x.stride(1) != 1 and x.shape[1] > 1:
            x = x.contiguous()
        return x

    @staticmethod
    def _wave_out(out, like, cols):
        import torch
        if out is None:
            return torch.empty((like.shape[0], cols), device=like.device, dtype=like.dtype)
        if (not isinstance(out, torch.Tensor) or out.dtype != like.dtype or out.device != like.device
                or tuple(out.shape) != (like.shape[0], cols) or out.stride(1) != 1):
            raise GtcrnError(f"out must be a {like.dtype} tensor of shape ({like.shape[0]}, {cols}) with contiguous rows")
        return out

    def _wave_call(self, name, state, x, out, rows, r=None):
        """gtcrn_wave_stream_<name>, or its _limited / _pcm16 twin, on checked rows: x holds a step's hops (r None) or a flush's
        tails of r samples; `rows` names the streams -- (slots, count, max_active) of a _slots call, in front of the samples,
        or (nstreams[, nhops]) behind them."""
        io = (x.data_ptr() if r != 0 else None, x.stride(0) if r != 0 else 0, *(() if r is None else (r,)), out.data_ptr(),
              out.stride(0))
        gain = () if state.dry_gain is None else (state.dry_gain.data_ptr(),)
        if name.endswith("_slots"):
            args = rows + io + (gain or (None,))
        else:
            args, name = io + rows + gain, name + ("_limited" if gain else "")
        self._bind_live(state)
        with self._dev():
            _check(_entry("gtcrn_wave_stream_" + name, x)(self._h, state.model.data_ptr(), state.wave.data_ptr(), *args,
                                                          state.window.data_ptr(), _stream_ptr()))
        return out

    def wave_stream_step(self, state, x, out=None):
        """x (N, 256*nhops) float32 or int16 -> the enhanced (N, 256*nhops), same dtype, one hop late (call 0 of a
        stream emits zeros).  Asynchronous on the current stream; no allocation when `out` is given and
        reserve(N, nhops) was called (capturable)."""
        x = self._wave_rows(state, x, "x")
        L = x.shape[1]
        if L < 256 or L % 256:
            raise GtcrnError(f"x must hold a whole number of 256-sample hops per stream, got {L}")
        return self._wave_call("step", state, x, self._wave_out(out, x, L), (state.n, L // 256))

    def wave_stream_flush(self, state, tail, out=None):
        """tail (N, r) float32 or int16, r = 0..255: the samples after the last whole hop -> the last 256 enhanced
        samples of every stream.  Ends the streams (reset them before reuse)."""
        tail = self._wave_rows(state, tail, "tail")
        r = tail.shape[1]
        if r > 255:
            raise GtcrnError(f"the tail holds 0..255 samples, got {r}: push whole hops with wave_stream_step first")
        return self._wave_call("flush", state, tail, self._wave_out(out, tail, 256), (state.n,), r)

    # ---- stream slots (contract: include/gtcrn_micro_hip.h, "stream slots") ------------------------------------------
    def _slot_args(self, slots, count, max_active):
        """Checks the slot table of a call: `slots` int32 (M,) on the model's device, `count` None or a one-element int32
        tensor there, max_active None (all M rows) or 1..M.  Nothing is read back: ids in range and distinct are the
        caller's precondition (check_slots verifies a list, synchronously)."""
        import torch
        if not isinstance(slots, torch.Tensor) or slots.dtype != torch.int32 or not slots.is_cuda or slots.device.index != self.device:
            raise GtcrnError(f"slots must be an int32 tensor on cuda:{self.device}")
        if slots.dim() != 1 or slots.numel() < 1 or not slots.is_contiguous():
            raise GtcrnError(f"slots must be a contiguous 1-D tensor, got shape {tuple(slots.shape)}")
        m = slots.numel() if max_active is None else int(max_active)
        if not 1 <= m <= slots.numel():
            raise GtcrnError(f"max_active must be 1..{slots.numel()} (the rows of slots), got {m}")
        if count is not None and (not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or count.numel() != 1
                                  or not count.is_cuda or count.device.index != self.device):
            raise GtcrnError(f"count must be a one-element int32 tensor on cuda:{self.device}")
        return m, (count.data_ptr() if count is not None else None)

    def check_slots(self, state, slots, count=None):
        """SYNCHRONOUS debugging validator: copies `slots` (and `count`) to the host and raises GtcrnError on an id outside
        0..n-1 or a repeated one among the rows that would step.  Launches nothing."""
        n = state.n if isinstance(state, WaveStreamState) else int(state.shape[0])
        self._slot_args(slots, count, None)
        ids = slots.detach().cpu().numpy()
        k = len(ids) if count is None else min(max(int(count.detach().cpu().reshape(-1)[0]), 0), len(ids))
        ids = ids[:k]
        bad = ids[(ids < 0) | (ids >= n)]
        if bad.size:
            raise GtcrnError(f"slot id {int(bad[0])} outside [0, {n})")
        uniq, cnt = np.unique(ids, return_counts=True)
        if (cnt > 1).any():
            raise GtcrnError(f"slot id {int(uniq[cnt > 1][0])} is named more than once")
        return k

    def stream_step_slots(self, state, slots, spec_t, count=None, out=None, max_active=None):
        """One frame for the rows a call names: spec_t (M,257,1,2), row i = the stream in slot slots[i] of `state`
        (new_state); `count` (device int32, None: all) rows step.  Returns (M,257,1,2); rows at or beyond count are not
        written."""
        import torch
        self._check_on_device(spec_t, "spec")
        if spec_t.dim() != 4 or spec_t.shape[1] != NBINS or spec_t.shape[2] != 1 or spec_t.shape[3] != 2:
            raise GtcrnError(f"spec must be (M,257,1,2), got {tuple(spec_t.shape)}")
        m, cnt = self._slot_args(slots, count, max_active)
        if spec_t.shape[0] != m:
            raise GtcrnError(f"spec must hold max_active = {m} rows, got {spec_t.shape[0]}")
        if spec_t.stride(3) != 1:
            spec_t = spec_t.contiguous()
        self._check_on_device(state, "state", (state.shape[0], self.state_bytes() // 4))
        if out is None:
            out = torch.empty((m, NBINS, 1, 2), device=spec_t.device, dtype=torch.float32)
        else:
            self._check_on_device(out, "out")
            if tuple(out.shape) != (m, NBINS, 1, 2) or out.stride(3) != 1:
                raise GtcrnError(f"out must be ({m},257,1,2) with contiguous re/im pairs, got {tuple(out.shape)}")
        isb, isf, ist = _spec_strides(spec_t)
        osb, osf, ost = _spec_strides(out)
        with self._dev():
            _check(lib().gtcrn_stream_step_slots(self._h, state.data_ptr(), slots.data_ptr(), cnt, m, spec_t.data_ptr(), isb, isf,
                                                 ist, out.data_ptr(), osb, osf, ost, _stream_ptr()))
        return out

    def _slot_rows(self, state, slots, x, count, max_active, what, cols=None):
        import torch
        if type(state) is not WaveStreamState:
            raise GtcrnError("slots= needs a state of new_wave_state: rate and packet streams share a group phase and "
                             "cannot be stepped by slot")
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in (torch.float32, torch.int16):
            raise GtcrnError(f"{what} must be a float32 or int16 CUDA (ROCm) tensor")
        if x.device.index != self.device or state.model.device != x.device:
            raise GtcrnError(f"{what} and the state must be on cuda:{self.device}")
        m, cnt = self._slot_args(slots, count, max_active)
        if x.dim() != 2 or x.shape[0] != m:
            raise GtcrnError(f"{what} must hold max_active = {m} rows, got {tuple(x.shape)}")
        if cols is not None and x.shape[1] != cols:
            raise GtcrnError(f"{what} must hold {cols} samples per row (one hop per call), got {x.shape[1]}")
        if x.stride(1) != 1 and x.shape[1] > 1:
            x = x.contiguous()
        return x, m, cnt

    def wave_stream_step_slots(self, state, slots, x, count=None, out=None, max_active=None):
        """One hop for the rows a call names: x (M, 256) float32 or int16, row i = the stream in slot slots[i] of `state`
        -> (M, 256), same dtype, each stream one hop late.  Applies state.dry_gain (per slot) when set.  Asynchronous; no
        allocation when `out` is given and reserve(M, 1) was called (capturable)."""
        x, m, cnt = self._slot_rows(state, slots, x, count, max_active, "x", 256)
        return self._wave_call("step_slots", state, x, self._wave_out(out, x, 256), (slots.data_ptr(), cnt, m))

    def wave_stream_flush_slots(self, state, slots, tail, count=None, out=None, max_active=None):
        """tail (M, r), r = 0..255: the samples after the last whole hop of the named streams -> their last 256 enhanced
        samples.  Ends those streams (wave_stream_reset_slots before a slot is reused); the others are not touched."""
        tail, m, cnt = self._slot_rows(state, slots, tail, count, max_active, "tail")
        r = tail.shape[1]
        if r > 255:
            raise GtcrnError(f"the tail holds 0..255 samples, got {r}: push whole hops with wave_stream_step_slots first")
        return self._wave_call("flush_slots", state, tail, self._wave_out(out, tail, 256), (slots.data_ptr(), cnt, m), r)

    def wave_stream_reset_slots(self, state, slots, count=None, max_active=None):
        """Resets the named slots (both states) to the start of a new clip, with a kernel: asynchronous and capturable."""
        if type(state) is not WaveStreamState:
            raise GtcrnError("slots= needs a state of new_wave_state")
        m, cnt = self._slot_args(slots, count, max_active)
        with self._dev():
            _check(lib().gtcrn_stream_reset_slots(self._h, state.model.data_ptr(), state.wave.data_ptr(), slots.data_ptr(), cnt, m,
                                                  _stream_ptr()))

    # ---- other sample rates (contract: include/gtcrn_micro_hip.h, gtcrn_resample / gtcrn_rate_stream_*) -------------
    def resampler(self, fs_in, fs_out):
        """The Resampler fs_in -> fs_out on this model's device, made once per pair."""
        cache = self.__dict__.setdefault("_resamplers", {})
        key = (int(fs_in), int(fs_out))
        if key not in cache:
            cache[key] = Resampler(key[0], key[1], self.device)
        return cache[key]

    def forward_wave_rate(self, wave, fs, window, out_fs=None, dry_gain=None, highband=None, lengths=None):
        """wave (B,L) or (L,) at `fs` Hz -> the enhanced waveform at 16 kHz (out_fs None or 16000) or at `out_fs`: exactly
        resampler(fs, 16000)(wave) -> forward_wave -> resampler(16000, out_fs), the three public calls composed.
        dry_gain goes to forward_wave: the attenuation limit is mixed at 16 kHz.
        highband (None, a float or a (B,) CUDA float tensor, each in [0, 1]; fs = out_fs in 24000, 32000, 48000): the
        header's "high band", offline form -- the last call becomes gtcrn_resample_hb, which resamples
        fl(y - fl(gamma x16)) and adds fl(gamma wave[j]) for j < L: the band above 8 kHz comes out with gain gamma.
        lengths (B ints, with highband only): row b holds lengths[b] samples; forward_wave_var runs in the middle and the
        output row carries the samples of that clip alone, zeros behind them."""
        fs = int(fs)
        if highband is not None:
            return self._forward_wave_rate_hb(wave, fs, window, out_fs, dry_gain, highband, lengths)
        if lengths is not None:
            raise GtcrnError("lengths= is taken with highband= only")
        x = wave if fs == 16000 else self.resampler(fs, 16000)(wave)
        y = self.forward_wave(x, window, dry_gain=dry_gain)
        if out_fs is None or int(out_fs) == 16000:
            return y
        return self.resampler(16000, int(out_fs))(y)

    def _forward_wave_rate_hb(self, wave, fs, window, out_fs, dry_gain, highband, lengths):
        import torch
        if fs not in HIGHBAND_RATES or out_fs is None or int(out_fs) != fs:
            raise GtcrnError(f"highband= needs fs == out_fs in {HIGHBAND_RATES}, got fs {fs} out_fs {out_fs}")
        self._check_on_device(wave, "wave")
        w2 = (wave.reshape(1, -1) if wave.dim() == 1 else wave).contiguous()
        if w2.dim() != 2:
            raise GtcrnError(f"wave must be (B,L) or (L,), got {tuple(wave.shape)}")
        B, L = w2.shape
        gamma = self._dry_gain(highband, B, w2.device)               # (the same checks: [0, 1], (B,) float32 on the device)
        down, up = self.resampler(fs, 16000), self.resampler(16000, fs)
        if lengths is None:
            xlens = lens16 = None
            x16 = down(w2)
            y = self.forward_wave(x16, window, dry_gain=dry_gain)
        else:
            xl = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).cpu()
            if xl.numel() != B or int(xl.min()) < 0 or int(xl.max()) > L:
                raise GtcrnError(f"lengths must hold {B} entries in [0, L={L}]")
            l16 = torch.tensor([down.out_len(int(v)) for v in xl], dtype=torch.int32)
            x16 = torch.zeros((B, down.out_len(L)), device=w2.device, dtype=torch.float32)
            down(w2, lengths=xl, out=x16)
            y = self.forward_wave_var(x16, l16, window, dry_gain=dry_gain)
            xlens = xl.to(device=w2.device, dtype=torch.int32)
            lens16 = (256 * (l16 // 256)).to(device=w2.device, dtype=torch.int32)
        L16 = y.shape[1]
        if L16 < 1:
            raise GtcrnError("the clip holds less than one hop at 16 kHz")
        n = up.out_len(L16)
        out = torch.zeros((B, n), device=w2.device, dtype=torch.float32)
        with self._dev():
            _check(lib().gtcrn_resample_hb(up._h, y.data_ptr(), y.stride(0), x16.data_ptr(), x16.stride(0),
                                           lens16.data_ptr() if lens16 is not None else None, L16, w2.data_ptr(), w2.stride(0),
                                           xlens.data_ptr() if xlens is not None else None, L, gamma.data_ptr(),
                                           out.data_ptr(), out.stride(0), B, _stream_ptr()))
        return out[0] if wave.dim() == 1 else out

    def new_rate_state(self, nstreams, window, fs, atten_lim_db=None, meters=False, highband=None, ramp=False, alc=None,
                       tones=None):
        """State of `nstreams` live streams at `fs` Hz (8000, 24000, 32000 or 48000): new_wave_state's plus the two
        resamplers and their per-stream histories.  atten_lim_db: as in new_wave_state (mixed at 16 kHz); meters: as in
        new_wave_state (taken at 16 kHz, per 256-sample block of the wave step); ramp: as in new_wave_state (made at 16 kHz,
        over one 256-sample block of the wave step).  highband (a float or one per stream, each
        in [0, 1]; fs = 24000, 32000 or 48000; None: off, the plain calls): the header's "high band" -- the state gets
        ``hb`` (N, rate_stream_hb_state_bytes/4) and the per-stream gains ``hb_gain`` that every step then applies
        (RateStreamState.set_highband_gain rewrites them in place).  alc: as in new_wave_state (made at 16 kHz, per block of
        the wave step); not together with highband=."""
        import torch
        _alc_without_highband(alc, highband)
        fs = int(fs)
        hop = _check(lib().gtcrn_rate_stream_hop(fs))
        nhb = rate_stream_hb_state_bytes(fs) // 4 if highband is not None else 0        # (raises without a high band at fs)
        ws = self.new_wave_state(nstreams, window, meters=meters)
        st = RateStreamState(ws.model, ws.wave, ws.window, fs, hop, self.resampler(fs, 16000), self.resampler(16000, fs),
                             torch.empty((ws.n, rate_stream_state_bytes(fs) // 4), device=ws.wave.device, dtype=torch.float32))
        if highband is not None:
            st.hb = torch.empty((ws.n, nhb), device=ws.wave.device, dtype=torch.float32)
            st.hb_gain = torch.zeros((ws.n,), device=ws.wave.device, dtype=torch.float32)
            st.set_highband_gain(highband)
        self.rate_stream_reset(st)
        return _attach_live(st, atten_lim_db, ws.meters, ramp, alc, tones)

    def rate_stream_reserve(self, state, nhops):
        """Sizes every buffer a rate step of `nhops` hops needs: after it a step allocates nothing (capturable)."""
        _check(lib().gtcrn_rate_stream_reserve(self._h, state.rs_in._h, state.rs_out._h, state.n, int(nhops)))

    def rate_stream_reset(self, state, lo=0, hi=None):
        """Resets streams lo..hi-1 (all three states) to the start of a new clip."""
        if not isinstance(state, RateStreamState):
            raise GtcrnError("state must come from new_rate_state")
        lo, hi = _stream_range(state.n, lo, hi)
        with self._dev():
            _check(lib().gtcrn_rate_stream_reset(self._h, state.rs_in._h, state.rs_out._h, state.model[lo:hi].data_ptr(),
                                                 state.wave[lo:hi].data_ptr(), state.rate[lo:hi].data_ptr(), hi - lo,
                                                 _stream_ptr()))
            if state.hb is not None:
                _check(lib().gtcrn_rate_stream_hb_reset(state.fs, state.hb[lo:hi].data_ptr(), hi - lo, _stream_ptr()))

    def rate_stream_step(self, state, x, out=None):
        """x (N, H*nhops) float32 or int16 at the state's rate (H = state.hop) -> the enhanced (N, H*nhops) at that rate,
        same dtype, state.latency samples late.  Asynchronous on the current stream; no allocation when `out` is given
        and rate_stream_reserve(state, nhops) was called.  A state with highband= runs gtcrn_rate_stream_step_hb: `out`
        must not overlap x (the call is not legal in place)."""
        if not isinstance(state, RateStreamState):
            raise GtcrnError("state must come from new_rate_state")
        x = self._wave_rows(state, x, "x")
        L = x.shape[1]
        if L < state.hop or L % state.hop:
            raise GtcrnError(f"x must hold a whole number of {state.hop}-sample hops per stream, got {L}")
        out = self._wave_out(out, x, L)
        args = (self._h, state.rs_in._h, state.rs_out._h, state.model.data_ptr(), state.wave.data_ptr(),
                state.rate.data_ptr(), x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), state.n, L // state.hop)
        win, gain = state.window.data_ptr(), None if state.dry_gain is None else state.dry_gain.data_ptr()
        self._bind_live(state)
        with self._dev():
            if state.hb is not None:
                _check(_entry("gtcrn_rate_stream_step_hb", x)(*args, gain, win, state.hb.data_ptr(), state.hb_gain.data_ptr(),
                                                              _stream_ptr()))
            elif gain is None:
                _check(_entry("gtcrn_rate_stream_step", x)(*args, win, _stream_ptr()))
            else:
                _check(_entry("gtcrn_rate_stream_step_limited", x)(*args, gain, win, _stream_ptr()))
        return out

    def rate_stream_handoff(self, state, nhops, which=0):
        """Test hook: a copy of the 16 kHz hand-off of the most recent rate step of `nhops` hops, (N, 256*nhops): which = 0
        what k_rate_in produced, 1 what the wave step produced."""
        import torch
        out = torch.empty((state.n, 256 * int(nhops)), device=state.wave.device, dtype=torch.float32)
        with self._dev():
            _check(lib().gtcrn_rate_stream_debug_handoff(self._h, int(which), out.data_ptr(), out.numel(), _stream_ptr()))
        return out

    # ---- packet-sized live streaming (contract: include/gtcrn_micro_hip.h, gtcrn_packet_stream_*) -------------------
    def new_packet_state(self, nstreams, window, packet, fs=16000, atten_lim_db=None, meters=False, g711=None,
                         highband=None, ramp=False, alc=None, tones=None):
        """State of a GROUP of `nstreams` live streams whose audio arrives in packets of `packet` samples at `fs` Hz (8000,
        16000, 22050, 24000, 32000, 44100 or 48000; packet * 16000 / fs a whole number in 1..4096): new_wave_state's plus
        the two FIFOs and filter histories per stream and the host handle that holds the group's phase.  Everything a step
        needs is reserved here.  atten_lim_db: as in new_wave_state; the handle keeps the gains' address
        (gtcrn_packet_stream_set_dry_gain), so a captured period follows later changes of the gains.  meters: as in
        new_wave_state (taken at 16 kHz, per 256-sample block of the wave step; a call without a hop leaves them alone).
        ramp: as in new_wave_state (made at 16 kHz over one block of the wave step; a call without a hop leaves the words alone).
        g711: "ulaw", "alaw" or None -- the law of the torch.uint8 rows packet_stream_step then takes and returns (RTP payload
        types 0 / 8; float32 and int16 rows stay legal); without a law uint8 rows are refused.
        highband (a float or one per stream, each in [0, 1]; fs = 24000, 32000 or 48000 and a latency that is whole at fs;
        None: off, the plain calls): the header's "high band on the packet forms" -- the state gets ``hb``
        (N, packet_stream_hb_state_bytes / 4), the per-stream gains ``hb_gain`` every step then applies
        (set_highband_gain rewrites them in place) and ``hb_latency`` in samples at fs; not together with g711=.
        alc: as in new_wave_state (made at 16 kHz, per block of the wave step; a call without a hop leaves the records alone);
        not together with highband=."""
        import torch
        _alc_without_highband(alc, highband)
        law = g711_law(g711)
        fs, packet = int(fs), int(packet)
        n16 = packet_stream_n16(fs, packet)
        nbytes = packet_stream_state_bytes(fs, packet)
        nhb = _packet_hb_floats(fs, packet, highband, law)
        ws = self.new_wave_state(nstreams, window, meters=meters)
        rs_in = self.resampler(fs, 16000) if fs != 16000 else None
        rs_out = self.resampler(16000, fs) if fs != 16000 else None
        h = ctypes.c_void_p()
        with self._dev():
            _check(lib().gtcrn_packet_stream_create(ctypes.byref(h), self._h, rs_in._h if rs_in else None,
                                                    rs_out._h if rs_out else None, fs, packet, ws.n))
        st = PacketStreamState(self, h, ws.model, ws.wave, ws.window, fs, packet, n16, rs_in, rs_out,
                               torch.empty((ws.n, nbytes // 4), device=ws.wave.device, dtype=torch.float32))
        st.g711 = law
        st._new_highband(nhb, highband)
        self.packet_stream_reset(st)
        return _attach_live(st, atten_lim_db, ws.meters, ramp, alc, tones)

    def packet_stream_reset(self, state, lo=0, hi=None):
        """Resets streams lo..hi-1 (all three states).  They join the group at its current phase: state.phase zeros in
        front of their input, the group's latency."""
        if not isinstance(state, PacketStreamState) or isinstance(state, PacketSlotState):
            raise GtcrnError("state must come from new_packet_state")
        lo, hi = _stream_range(state.n, lo, hi)
        with self._dev():
            _check(lib().gtcrn_packet_stream_reset(state._h, state.model[lo:hi].data_ptr(), state.wave[lo:hi].data_ptr(),
                                                   state.pkt[lo:hi].data_ptr(), hi - lo, _stream_ptr()))
            if state.hb is not None:
                _check(lib().gtcrn_packet_stream_hb_reset(state._h, state.hb[lo:hi].data_ptr(), hi - lo, _stream_ptr()))

    def packet_stream_step(self, state, x, out=None):
        """x (N, state.packet) float32 or int16 at the state's rate -> the enhanced (N, state.packet), same dtype,
        state.latency16 samples (counted at 16 kHz) late.  Steps state.next_hops hops of the model (possibly none) and
        advances the group's phase.  Asynchronous on the current stream; no allocation when `out` is given.  On a state
        made with g711=, x may be torch.uint8: G.711 codes of that law in, codes out (gtcrn_packet_stream_step_g711).  A
        state with highband= runs gtcrn_packet_stream_step_hb: `out` must not overlap x (the call is not legal in place)."""
        import torch
        if not isinstance(state, PacketStreamState) or isinstance(state, PacketSlotState):
            raise GtcrnError("state must come from new_packet_state")
        _g711_rows(state, x, "x")
        x = self._wave_rows(state, x, "x", g711=True)
        if x.shape[1] != state.packet:
            raise GtcrnError(f"x must hold one packet of {state.packet} samples per stream, got {x.shape[1]}")
        out = self._wave_out(out, x, state.packet)
        fn = _entry("gtcrn_packet_stream_step", x)
        law = (state.g711,) if x.dtype == torch.uint8 else ()
        if law:
            fn = lib().gtcrn_packet_stream_step_g711
        hb = ()
        if state.hb is not None:
            fn = _entry("gtcrn_packet_stream_step_hb", x)
            hb = (state.hb.data_ptr(), state.hb_gain.data_ptr())
        state.last_hops = state.next_hops
        self._bind_live(state)
        with self._dev():
            # (a one-row tensor may report any stride)
            _check(fn(state._h, state.model.data_ptr(), state.wave.data_ptr(), state.pkt.data_ptr(), x.data_ptr(),
                      max(x.stride(0), state.packet), out.data_ptr(), max(out.stride(0), state.packet), state.n, *law,
                      state.window.data_ptr(), *hb, _stream_ptr()))
        return out

    def packet_stream_handoff(self, state, which=0):
        """Test hook: a copy of the 16 kHz hand-off of the most recent packet step, (N, 256 * hops of that step): which = 0
        what k_packet_in produced, 1 what the wave step produced."""
        import torch
        out = torch.empty((state.n, 256 * state.last_hops), device=state.wave.device, dtype=torch.float32)
        if out.numel():
            with self._dev():
                _check(lib().gtcrn_packet_stream_debug_handoff(state._h, int(which), out.data_ptr(), out.numel(),
                                                               _stream_ptr()))
        return out

    # ---- packet stream slots (contract: include/gtcrn_micro_hip.h, "packet stream slots") ----------------------------
    def new_packet_slot_state(self, nslots, window, packet, fs=16000, max_active=None, atten_lim_db=None, meters=False,
                              g711=None, highband=None, ramp=False, alc=None, tones=None):
        """State of `nslots` RESIDENT packet streams, each with its own phase: new_packet_state's tensors for nslots streams
        plus ``phase`` (nslots,) int32 on the device.  A call steps the at most `max_active` (None: nslots) slots it names
        (packet_stream_step_slots); streams join by packet_stream_reset_slots, at any tick, and all have the latency of a
        one-stream group created at phase 0.  Everything a step needs is reserved here.  atten_lim_db and meters: as in
        new_wave_state, per SLOT; ramp likewise.  g711: as in new_packet_state.  highband: as in new_packet_state, one gain per SLOT;
        packet_stream_reset_slots then zeroes the named slots' rows of ``hb`` too.  alc: as in new_packet_state, one record
        per SLOT."""
        import torch
        _alc_without_highband(alc, highband)
        law = g711_law(g711)
        fs, packet = int(fs), int(packet)
        n16 = packet_stream_n16(fs, packet)
        nbytes = packet_stream_state_bytes(fs, packet)
        nhb = _packet_hb_floats(fs, packet, highband, law)
        ws = self.new_wave_state(nslots, window, meters=meters)
        m = ws.n if max_active is None else int(max_active)
        if not 1 <= m <= ws.n:
            raise GtcrnError(f"max_active must be 1..{ws.n} (the resident slots), got {m}")
        rs_in = self.resampler(fs, 16000) if fs != 16000 else None
        rs_out = self.resampler(16000, fs) if fs != 16000 else None
        h = ctypes.c_void_p()
        with self._dev():
            _check(lib().gtcrn_packet_stream_create(ctypes.byref(h), self._h, rs_in._h if rs_in else None,
                                                    rs_out._h if rs_out else None, fs, packet, m))
        st = PacketSlotState(self, h, ws.model, ws.wave, ws.window, fs, packet, n16, rs_in, rs_out,
                             torch.zeros((ws.n, nbytes // 4), device=ws.wave.device, dtype=torch.float32),
                             torch.zeros((ws.n,), device=ws.wave.device, dtype=torch.int32), m)
        st.g711 = law
        st._new_highband(nhb, highband)
        if st.hb is not None:
            st.hb.zero_()
        return _attach_live(st, atten_lim_db, ws.meters, ramp, alc, tones)

    def _packet_slot_args(self, state, slots, count):
        if not isinstance(state, PacketSlotState):
            raise GtcrnError("state must come from new_packet_slot_state")
        m, cnt = self._slot_args(slots, count, None)
        if m > state.max_active:
            raise GtcrnError(f"slots holds {m} rows, the state was made for max_active = {state.max_active}")
        return m, cnt

    def packet_stream_step_slots(self, state, slots, x, count=None, out=None):
        """One packet for the rows a call names: x (M, state.packet) float32 or int16 (or, on a state made with g711=,
        torch.uint8 G.711 codes: gtcrn_packet_stream_step_slots_g711) at the state's rate, row i = the
        stream in slot slots[i] (int32 device tensor, M <= state.max_active ids, in range and distinct); `count` (device
        int32, None: all M) rows step.  Returns (M, state.packet), same dtype, state.latency16 samples (at 16 kHz) late per
        stream; rows at or beyond count are not written and no other slot is touched.  The launch sequence is the same
        for every call: asynchronous, capturable, no allocation when `out` is given.  A state with highband= runs
        gtcrn_packet_stream_step_slots_hb: `out` must not overlap x."""
        import torch
        if isinstance(state, PacketSlotState):
            _g711_rows(state, x, "x")
        m, cnt = self._packet_slot_args(state, slots, count)
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in (torch.float32, torch.int16, torch.uint8):
            raise GtcrnError("x must be a float32 or int16 CUDA (ROCm) tensor (uint8 G.711 codes on a state made with g711=)")
        if x.device.index != self.device or state.model.device != x.device:
            raise GtcrnError(f"x and the state must be on cuda:{self.device}")
        if x.dim() != 2 or tuple(x.shape) != (m, state.packet):
            raise GtcrnError(f"x must be ({m}, {state.packet}): one packet per row of slots, got {tuple(x.shape)}")
        if x.stride(1) != 1:
            x = x.contiguous()
        out = self._wave_out(out, x, state.packet)
        fn = _entry("gtcrn_packet_stream_step_slots", x)
        law = (state.g711,) if x.dtype == torch.uint8 else ()
        if law:
            fn = lib().gtcrn_packet_stream_step_slots_g711
        hb = ()
        if state.hb is not None:
            fn = _entry("gtcrn_packet_stream_step_slots_hb", x)
            hb = (state.hb.data_ptr(), state.hb_gain.data_ptr())
        self._bind_live(state)
        with self._dev():
            # (a one-row tensor may report any stride)
            _check(fn(state._h, state.model.data_ptr(), state.wave.data_ptr(), state.pkt.data_ptr(), state.phase.data_ptr(),
                      slots.data_ptr(), cnt, m, x.data_ptr(), max(x.stride(0), state.packet), out.data_ptr(),
                      max(out.stride(0), state.packet), *law, state.window.data_ptr(), *hb, _stream_ptr()))
        return out

    def packet_stream_reset_slots(self, state, slots, count=None):
        """Resets the named slots (all three states and the phase word) to the start of a new clip, with kernels:
        asynchronous and capturable.  The streams join at phase 0 whatever the other slots' phases are."""
        m, cnt = self._packet_slot_args(state, slots, count)
        with self._dev():
            _check(lib().gtcrn_packet_stream_reset_slots(state._h, state.model.data_ptr(), state.wave.data_ptr(),
                                                         state.pkt.data_ptr(), state.phase.data_ptr(), slots.data_ptr(), cnt, m,
                                                         _stream_ptr()))
            if state.hb is not None:
                _check(lib().gtcrn_packet_stream_hb_reset_slots(state._h, state.hb.data_ptr(), slots.data_ptr(), cnt, m,
                                                                _stream_ptr()))

    def _cache_ptrs(self, tcn_cache):
        flat = [tcn_cache[g][k] for g in range(2) for k in range(4)]
        for g in range(2):
            for k in range(4):
                _require_cuda_f32(tcn_cache[g][k], "tcn_cache")
                assert tcn_cache[g][k].is_contiguous()
        arr = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in flat])
        return arr

    def stream_import(self, state, conv_cache, tra_cache, tcn_cache):
        N = state.shape[0]
        assert conv_cache.is_contiguous() and tra_cache.is_contiguous()
        with self._dev():
            _check(lib().gtcrn_stream_import(self._h, state.data_ptr(), N, conv_cache.data_ptr(),
                                             tra_cache.data_ptr(), self._cache_ptrs(tcn_cache), _stream_ptr()))

    def stream_export(self, state, conv_cache, tra_cache, tcn_cache):
        N = state.shape[0]
        assert conv_cache.is_contiguous() and tra_cache.is_contiguous()
        with self._dev():
            _check(lib().gtcrn_stream_export(self._h, state.data_ptr(), N, conv_cache.data_ptr(),
                                             tra_cache.data_ptr(), self._cache_ptrs(tcn_cache), _stream_ptr()))

    # ---- test / measurement hooks ------------------------------------------------------------
    def debug_enable(self, on=True):
        """True / 1: stage taps (and phase stamps in the diagnostic build); 2: phase stamps only (single-frame streaming
        steps keep their one-launch form)."""
        _check(lib().gtcrn_debug_enable(self._h, 2 if on == 2 else int(bool(on))))

    def var_spans_enable(self, on=True):
        """Variable-length batches in time spans (default on; results are bit-identical either way -- the A/B switch)."""
        _check(lib().gtcrn_var_spans_enable(self._h, int(bool(on))))

    def stream_form(self, form=0):
        """Single-frame streaming steps: 0 = one launch per step, four or seven streams per workgroup by the stream count
        (default); 1 = the three-launch form; 2 / 3 = one launch pinned to four / seven streams per workgroup (A/B
        switches; bit-identical results)."""
        _check(lib().gtcrn_stream_form(self._h, int(form)))

    def tap(self, name, b, T):
        """Stage tap of clip b of the most recent forward, (C,T,F) float32: en0..en4, gtcn1, gtcn2 (fp32 forwards
        only), sum4 (gtcn2 + en4 as stored: the decoder's first input), and -- with debug_enable before the forward --
        de0..de4.  After a quant forward (which needs debug_enable for every tap) the values are the fp16 records,
        widened."""
        F = {"en0": 65, "de3": 65}.get(name, 33)
        shape = (2, T, 129) if name == "de4" else (16, T, F)
        dst = np.empty(shape, np.float32)
        n = lib().gtcrn_debug_tap(self._h, name.encode(), int(b), dst.ctypes.data_as(_c_f32p), dst.size)
        _check(n)
        assert n == dst.size, (n, dst.size)
        return dst

    def stamps(self, kernel, B):
        """Diagnostic build: (B,16) phase cycle sums of kernel 0 encoder, 1 gtcn1, 2 gtcn2, 3 decoder."""
        dst = np.zeros((B, 16), np.uint64)
        _check(lib().gtcrn_debug_stamps(self._h, int(kernel), dst.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)),
                                        dst.size))
        return dst

    _kernels = None

    @classmethod
    def kernel_names(cls):
        """The kernels the library times, in its own order (every timed launch records which one it was)."""
        if cls._kernels is None:
            buf = ctypes.create_string_buffer(64)
            ms, n = ctypes.c_float(), ctypes.c_int()
            names = []
            for i in range(lib().gtcrn_timing_kernels()):
                _check(lib().gtcrn_timing_read(None, -1 - i, buf, 64, ctypes.byref(ms), ctypes.byref(n)))
                names.append(buf.value.decode())
            cls._kernels = tuple(names)
        return cls._kernels

    def timing_enable(self, on=True, only=None):
        """HIP-event timing of the kernel launches; only="k_decoder" keeps the events of that kernel alone (an
        event pair costs a few microseconds of dispatch gap per launch)."""
        mode = 0 if not on else (1 if only is None else 2 + self.kernel_names().index(only))
        _check(lib().gtcrn_timing_enable(self._h, mode))

    def timing_read(self):
        """{kernel name: (average ms, launches)} over the launches recorded since timing_enable(True)."""
        out = {}
        buf = ctypes.create_string_buffer(64)
        ms, n = ctypes.c_float(), ctypes.c_int()
        for i in range(len(self.kernel_names())):
            _check(lib().gtcrn_timing_read(self._h, i, buf, 64, ctypes.byref(ms), ctypes.byref(n)))
            if n.value:
                out[buf.value.decode()] = (float(ms.value), int(n.value))
        return out


class WaveStreamState:
    """The device state of hop-level waveform streams (Engine.new_wave_state): ``model`` (N, state_bytes/4), the state of
    stream_step (importable / exportable as the reference's caches); ``wave`` (N, wave_state_bytes/4); and the checked
    512-tap ``window`` every step and flush of these streams uses."""

    def __init__(self, model, wave, window):
        self.model = model
        self.wave = wave
        self.window = window
        self.dry_gain = None        # (N,) float32 on the device: the attenuation limit's dry gains; None: limit off
        self.meters = None          # (N, 4) float32 on the device: {E_dry, E_out, peak, blocks} per stream; None: no metering
        self.gain_ramp = None       # (N,) float32 on the device: the dry gain each stream's last block ended at; None: no ramps
        self.alc = None             # (N, 8) float32 on the device: the level-control records; None: no level control
        self.alc_params = None      # (16,) float32 on the device: the level control's parameter words
        self.alc_fields = None      # the configuration the words were made from (gtcrn_alc_config's fields), as set_alc keeps it
        self.tones = None           # (N, 8) float32 on the device: the tone guard's records; None: no tone guard
        self.tone_params = None     # (16,) float32 on the device: the tone guard's parameter words
        self.tone_table = None      # (10, 256, 2) float32 on the device: the tone guard's table
        self.tone_fields = None     # the configuration the words were made from (gtcrn_tone_config's fields)

    @property
    def n(self):
        return self.model.shape[0]

    def set_dry_gain(self, gain):
        """Installs `gain`, a contiguous (N,) float32 tensor on the state's device holding every stream's dry gain in
        [0, 1] (the caller's precondition: it is not read back), or None: the limit off, the plain kernels again.  The
        steps read the tensor on the device at every call, so it may be rewritten in place at any time."""
        import torch
        if gain is not None and (not isinstance(gain, torch.Tensor) or gain.dtype != torch.float32 or gain.device != self.model.device
                                 or tuple(gain.shape) != (self.n,) or not gain.is_contiguous()):
            raise GtcrnError(f"the dry gains must be a contiguous ({self.n},) float32 tensor on {self.model.device}")
        self.dry_gain = gain

    def _new_gain_ramp(self):
        """ramp=True of the state's constructor: the ramp words, equal to the gains (zeros where the state has no limit)."""
        import torch
        if not hasattr(lib(), "gtcrn_wave_stream_set_gain_ramp"):
            raise GtcrnError("this library has no gain ramps")
        if self.dry_gain is None:
            self.set_dry_gain(torch.zeros((self.n,), device=self.model.device, dtype=torch.float32))
        self.gain_ramp = self.dry_gain.clone()

    def set_atten_lim_db(self, db, lo=0, hi=None, snap=False):
        """Sets the attenuation limit of streams lo..hi-1 to `db` dB (None or inf: no limit, 0: bypass; a sequence gives
        one limit per stream of the range): rewrites state.dry_gain[lo:hi] on the device, asynchronously on the current
        stream and, for one value, without any allocation; takes effect at the next emitted block, also under the replay of
        a captured graph.  A state created without a limit gets its gains (zeros: no limit) at the first call here.
        On a state made with ramp=True the change is spread over the next emitted block of each stream; snap=True also
        writes state.gain_ramp[lo:hi], so the change lands at once, as it does without ramps."""
        import torch
        lo, hi = _stream_range(self.n, lo, hi)
        g = _gains_of(db, hi - lo)
        if self.dry_gain is None:
            self.set_dry_gain(torch.zeros((self.n,), device=self.model.device, dtype=torch.float32))
        if isinstance(g, float):
            self.dry_gain[lo:hi].fill_(g)
        else:
            self.dry_gain[lo:hi].copy_(torch.from_numpy(g), non_blocking=True)
        if snap and self.gain_ramp is not None:
            self.gain_ramp[lo:hi].copy_(self.dry_gain[lo:hi])

    def _new_alc(self, alc):
        """alc= of the state's constructor: the parameter words and the records, every stream at its initial record."""
        import torch
        if not hasattr(lib(), "gtcrn_wave_stream_set_alc"):
            raise GtcrnError("this library has no level control")
        self.alc_fields = _alc_fields(alc)        # the configuration set_alc updates
        words = alc_params(**self.alc_fields)
        self.alc_params = torch.from_numpy(words).to(self.model.device)
        self.alc = torch.zeros((self.n, 8), device=self.model.device, dtype=torch.float32)
        self.reset_alc()

    def _leveled(self):
        if self.alc is None:
            raise GtcrnError("the state has no level control: create it with alc=")
        return self.alc

    def set_alc(self, **fields):
        """Replaces the given settings of the state's OWN configuration (``state.alc_fields``: what alc= gave, as later calls
        here left it -- an alc="vad" state stays measure-only unless mode=1 is passed) and rewrites state.alc_params in
        place, asynchronously on the current stream: the next step, also the next replay of a captured one, follows.
        Nothing changes when a setting is refused."""
        import torch
        self._leveled()
        merged = dict(self.alc_fields or ALC_DEFAULTS, **fields)
        words = alc_params(**merged)
        self.alc_fields = merged
        self.alc_params.copy_(torch.from_numpy(words), non_blocking=True)

    def reset_alc(self, lo=0, hi=None):
        """Writes the initial record {1, 0, 0, 0, 0, 0, 0, 0} to streams (slots) lo..hi-1, asynchronously on the current stream
        and without any allocation.  (A stream's first block does the same on the device: a join needs no call here.)"""
        a = self._leveled()
        lo, hi = _stream_range(self.n, lo, hi)
        a[lo:hi].zero_()
        a[lo:hi, 0].fill_(1.0)

    def voice(self):
        """The voice flag of every stream's last emitted block: an (N,) bool tensor on the device, a compare of word 3 of the
        records.  Asynchronous, no synchronisation: usable inside a captured graph."""
        return self._leveled()[:, 3] != 0

    def alc_gain_db(self):
        """The gain every stream's last emitted block ended at, in dB: an (N,) float64 numpy array.  SYNCHRONOUS: word 0 of
        the records is copied to the host."""
        return 20.0 * np.log10(self._leveled()[:, 0].detach().cpu().numpy().astype(np.float64))

    def _new_tones(self, tones):
        """tones= of the state's constructor: the parameter words, the table and the records, every record zero."""
        import torch
        if not hasattr(lib(), "gtcrn_wave_stream_set_tone"):
            raise GtcrnError("this library has no tone guard")
        self.tone_fields = _tone_fields(tones)    # the configuration set_tones updates
        words = tone_params(**self.tone_fields)
        self.tone_params = torch.from_numpy(words).to(self.model.device)
        self.tone_table = torch.from_numpy(tone_table()).to(self.model.device)
        self.tones = torch.zeros((self.n, 8), device=self.model.device, dtype=torch.float32)

    def _toned(self):
        if self.tones is None:
            raise GtcrnError("the state has no tone guard: create it with tones=")
        return self.tones

    def set_tones(self, **fields):
        """Replaces the given settings of the state's OWN configuration (``state.tone_fields``: what tones= gave, as later
        calls here left it -- a tones="detect" state stays detect-only unless mode=1 is passed) and rewrites
        state.tone_params in place, asynchronously on the current stream: the next step, also the next replay of a captured
        one, follows.  Nothing changes when a setting is refused."""
        import torch
        self._toned()
        merged = dict(self.tone_fields or TONE_DEFAULTS, **fields)
        words = tone_params(**merged)
        self.tone_fields = merged
        self.tone_params.copy_(torch.from_numpy(words), non_blocking=True)

    def reset_tones(self, lo=0, hi=None):
        """Zeroes the records of streams (slots) lo..hi-1, asynchronously on the current stream and without any allocation.
        (A stream's first block does the same on the device: a join needs no call here.)"""
        t = self._toned()
        lo, hi = _stream_range(self.n, lo, hi)
        t[lo:hi].zero_()

    def tone(self):
        """The reported tone code of every stream's last emitted block (0 none, 1..16 = 1 + 4 row + col of the DTMF grid, 17 =
        1100 Hz, 18 = 2100 Hz): an (N,) int32 tensor on the device, a conversion of word 0 of the records.  Asynchronous, no
        synchronisation: usable inside a captured graph."""
        import torch
        return self._toned()[:, 0].to(torch.int32)

    def tone_events(self):
        """The reported onsets of every stream since its records were zeroed: an (N,) int64 numpy array.  SYNCHRONOUS: word 5
        of the records is copied to the host."""
        return self._toned()[:, 5].detach().cpu().numpy().astype(np.int64)

    def _metered(self):
        if self.meters is None:
            raise GtcrnError("the state has no level meters: create it with meters=True")
        return self.meters

    def reset_meters(self, lo=0, hi=None):
        """Starts a new window for streams (slots) lo..hi-1: zeroes their records, asynchronously on the current stream and
        without any allocation (a memset: capturable)."""
        m = self._metered()
        lo, hi = _stream_range(self.n, lo, hi)
        m[lo:hi].zero_()

    def levels(self):
        """The RFC 6464 audio level (0 loudest .. 127 silence, -dBov at full scale 1.0) of every stream's window since its
        last reset_meters, from E_out and 256 * blocks of the records: an (N,) int32 numpy array.  SYNCHRONOUS: the
        records (16 bytes per stream) are copied to the host."""
        rec = self._metered().detach().cpu().numpy().astype(np.float64)
        return level_dbov(rec[:, 1], 256.0 * rec[:, 3])


class RateStreamState(WaveStreamState):
    """WaveStreamState of live streams at ``fs`` Hz (Engine.new_rate_state): plus ``rate`` (N, rate_stream_state_bytes/4),
    the two resamplers, the hop ``hop`` = 256 fs / 16000 and the end-to-end ``latency``, both in samples at fs."""

    def __init__(self, model, wave, window, fs, hop, rs_in, rs_out, rate):
        super().__init__(model, wave, window)
        self.fs = fs
        self.hop = hop
        self.latency = rate_stream_latency(fs)
        self.rs_in = rs_in
        self.rs_out = rs_out
        self.rate = rate
        self.hb = None              # (N, rate_stream_hb_state_bytes/4): the high band's state; None: the plain calls
        self.hb_gain = None         # (N,) float32 on the device: the high-band gains

    def set_highband_gain(self, g):
        """Rewrites the high-band gains in place (a float for every stream, or N of them: a sequence or a tensor; each in
        [0, 1]), asynchronously on the current stream: the next step, also the next replay of a captured one, follows."""
        import torch
        if self.hb_gain is None:
            raise GtcrnError("the state has no high band: create it with highband=")
        if isinstance(g, torch.Tensor):
            if tuple(g.shape) != (self.n,):
                raise GtcrnError(f"the high-band gains must hold {self.n} values, got {tuple(g.shape)}")
            self.hb_gain.copy_(g.to(torch.float32), non_blocking=True)        # (a device tensor is not read back)
            return
        v = np.asarray(g, np.float32)
        if v.ndim > 1 or (v.ndim == 1 and v.size != self.n) or not np.all((v >= 0) & (v <= 1)):
            raise GtcrnError(f"the high-band gains must be one value or {self.n} of them, each in [0, 1]")
        if v.ndim == 0:
            self.hb_gain.fill_(float(v))
        else:
            self.hb_gain.copy_(torch.from_numpy(v), non_blocking=True)


class PacketStreamState(WaveStreamState):
    """WaveStreamState of a group of live streams fed in packets (Engine.new_packet_state): plus ``pkt``
    (N, packet_stream_state_bytes / 4: two FIFOs and the two filter histories per stream), the rate ``fs``, the packet
    ``packet`` in samples at fs and ``n16`` at 16 kHz, ``latency16`` (the end-to-end delay in 16 kHz samples; at fs it is
    latency16 * fs / 16000, not a whole number in the 44.1 kHz family), the host handle with the group's ``phase``, and
    ``g711`` (None, or the law 0 / 1 of the torch.uint8 rows the state takes)."""

    def __init__(self, engine, handle, model, wave, window, fs, packet, n16, rs_in, rs_out, pkt):
        super().__init__(model, wave, window)
        self._eng = engine          # the handle points into the engine's model and the resamplers: keep them alive
        self._h = handle
        self.fs = fs
        self.packet = packet
        self.n16 = n16
        self.latency16 = packet_stream_latency16(fs, packet)
        self.rs_in = rs_in
        self.rs_out = rs_out
        self.pkt = pkt
        self.last_hops = 0
        self.g711 = None            # the law of uint8 rows (0 mu-law, 1 A-law), or None: no uint8 rows
        self.hb = None              # (N, packet_stream_hb_state_bytes/4): the high band's state; None: the plain calls
        self.hb_gain = None         # (N,) float32 on the device: the high-band gains, per stream / slot
        self.hb_latency = None      # the end-to-end delay in samples at fs (whole wherever the high band exists)

    def _new_highband(self, nfloats, highband):
        import torch
        if highband is None:
            return
        self.hb = torch.empty((self.n, nfloats), device=self.wave.device, dtype=torch.float32)
        self.hb_gain = torch.zeros((self.n,), device=self.wave.device, dtype=torch.float32)
        self.hb_latency = packet_stream_hb_latency(self.fs, self.packet)
        self.set_highband_gain(highband)

    set_highband_gain = RateStreamState.set_highband_gain

    def set_dry_gain(self, gain):
        super().set_dry_gain(gain)
        _check(lib().gtcrn_packet_stream_set_dry_gain(self._h, None if gain is None else gain.data_ptr()))

    @property
    def phase(self):
        """(16 kHz samples the group has taken) mod 256."""
        return _check(lib().gtcrn_packet_stream_phase(self._h))

    @property
    def next_hops(self):
        """Hops of the model the next step runs (0 when the packet does not complete one)."""
        return _check(lib().gtcrn_packet_stream_next_hops(self._h))

    @property
    def period(self):
        """Calls after which the phase, and so the launch sequence, repeats: 256 / gcd(n16, 256)."""
        from math import gcd
        return 256 // gcd(self.n16, 256)

    def close(self):
        if getattr(self, "_h", None):
            lib().gtcrn_packet_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PacketSlotState(PacketStreamState):
    """PacketStreamState of RESIDENT packet streams with one phase each (Engine.new_packet_slot_state): ``phase`` is an
    (nslots,) int32 device tensor, slot s holding (16 kHz samples stream s has taken) mod 256, and ``max_active`` the most
    rows one call may name.  Stepped by Engine.packet_stream_step_slots only; the handle's host phase is not used."""

    phase = None                    # (an instance attribute here: the group's host phase of the base class does not apply)
    next_hops = None

    def __init__(self, engine, handle, model, wave, window, fs, packet, n16, rs_in, rs_out, pkt, phase, max_active):
        super().__init__(engine, handle, model, wave, window, fs, packet, n16, rs_in, rs_out, pkt)
        self.phase = phase
        self.max_active = max_active


SUPPORTED_RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
LIVE_RATES = (8000, 16000, 24000, 32000, 48000)
PACKET_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


def packet_stream_n16(fs, packet):
    """`packet` samples at `fs` Hz in 16 kHz samples (host only; raises for a packet the packet form does not take)."""
    return _check(lib().gtcrn_packet_stream_n16(int(fs), int(packet)))


def packet_stream_latency16(fs, packet):
    """End-to-end delay of the packet form in 16 kHz samples: 512 - gcd(n16, 256), plus the two filters' delays at
    fs != 16000 (host only)."""
    return _check(lib().gtcrn_packet_stream_latency16(int(fs), int(packet)))


def packet_stream_state_bytes(fs, packet):
    n = int(lib().gtcrn_packet_stream_state_bytes(int(fs), int(packet)))
    if n == 0:
        raise GtcrnError(lib().gtcrn_last_error().decode())
    return n


def packet_stream_hb_latency(fs, packet):
    """End-to-end delay in samples at `fs` of a packet form that carries the high band: packet_stream_latency16 * fs / 16000
    (host only; raises where there is no high band: 8 / 16 kHz, the 44.1 kHz family, 24 kHz with an odd n16)."""
    fn = getattr(lib(), "gtcrn_packet_stream_hb_latency", None)
    if fn is None:
        raise GtcrnError("this library has no high band on the packet forms")
    return _check(fn(int(fs), int(packet)))


def packet_stream_hb_state_bytes(fs, packet):
    """Bytes per stream of the packet forms' high-band state: 4 * (512 - gcd(n16, 256) + packet_stream_hb_latency), rounded
    up to a multiple of 16 (host only; raises where there is no high band)."""
    fn = getattr(lib(), "gtcrn_packet_stream_hb_state_bytes", None)
    if fn is None:
        raise GtcrnError("this library has no high band on the packet forms")
    n = int(fn(int(fs), int(packet)))
    if n == 0:
        raise GtcrnError(lib().gtcrn_last_error().decode())
    return n


def _packet_hb_floats(fs, packet, highband, law):
    """Floats per stream of ``hb`` for a packet state made with highband= (0 without), after the checks that need no device."""
    if highband is None:
        return 0
    if law is not None:
        raise GtcrnError("highband= and g711= exclude each other: G.711 is an 8 kHz payload and has no high band")
    return packet_stream_hb_state_bytes(fs, packet) // 4


def packet_stream_schedule(fs, packet, phase=0):
    """(hops, next phase) of a packet step taken at `phase` (host only)."""
    nxt = ctypes.c_int()
    h = _check(lib().gtcrn_packet_stream_schedule(int(fs), int(packet), int(phase), ctypes.byref(nxt)))
    return h, nxt.value


def resample_taps(fs_in, fs_out):
    """(up, down, h): the lowest-terms ratio fs_out / fs_in and the 2 half + 1 float32 coefficients the kernels use
    (host only; the filter's definition is in include/gtcrn_micro_hip.h)."""
    up, down = ctypes.c_int(), ctypes.c_int()
    n = _check(lib().gtcrn_resample_taps(int(fs_in), int(fs_out), ctypes.byref(up), ctypes.byref(down), None, 0))
    h = np.empty(n, np.float32)
    _check(lib().gtcrn_resample_taps(int(fs_in), int(fs_out), ctypes.byref(up), ctypes.byref(down),
                                     h.ctypes.data_as(_c_f32p), n))
    return up.value, down.value, h


def resample_out_len(fs_in, fs_out, L):
    return _check(lib().gtcrn_resample_out_len(int(fs_in), int(fs_out), int(L)))


def rate_stream_hop(fs):
    return _check(lib().gtcrn_rate_stream_hop(int(fs)))


def rate_stream_latency(fs):
    return _check(lib().gtcrn_rate_stream_latency(int(fs)))


def rate_stream_state_bytes(fs):
    n = int(lib().gtcrn_rate_stream_state_bytes(int(fs)))
    if n == 0:
        raise GtcrnError(lib().gtcrn_last_error().decode())
    return n


HIGHBAND_RATES = (24000, 32000, 48000)


def rate_stream_hb_state_bytes(fs):
    """Bytes per stream of the high band's state, 4 * (256 + latency) (host only; raises at a rate without a high band)."""
    fn = getattr(lib(), "gtcrn_rate_stream_hb_state_bytes", None)
    if fn is None:
        raise GtcrnError("this library has no high band")
    n = int(fn(int(fs)))
    if n == 0:
        raise GtcrnError(lib().gtcrn_last_error().decode())
    return n


class Resampler:
    """One polyphase resampler fs_in -> fs_out on one device (gtcrn_resampler): 16 kHz to or from 8, 11.025, 22.05, 24,
    32, 44.1 or 48 kHz.  Calling it resamples a (B,L) / (L,) float32 or int16 CUDA tensor."""

    def __init__(self, fs_in, fs_out, device=0):
        self.fs_in, self.fs_out, self.device = int(fs_in), int(fs_out), int(device)
        h = ctypes.c_void_p()
        _check(lib().gtcrn_resampler_create(ctypes.byref(h), self.fs_in, self.fs_out, self.device))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().gtcrn_resampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def out_len(self, L):
        return resample_out_len(self.fs_in, self.fs_out, L)

    def __call__(self, x, lengths=None, out=None, out_dtype=None):
        """x (B,L) or (L,): float32, or int16 PCM (then the output is float32).  lengths (optional, B ints, host or
        device): row b holds lengths[b] <= L samples and receives out_len(lengths[b]); the rest of its output row is left
        as it is.  out: a (B, >= out_len(L)) tensor with contiguous rows, float32 or (float32 input only) int16;
        out_dtype=torch.int16 asks for a new int16 output.  Asynchronous on the current stream."""
        import torch
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in (torch.float32, torch.int16):
            raise GtcrnError("x must be a float32 or int16 CUDA (ROCm) tensor")
        if x.device.index != self.device:
            raise GtcrnError(f"x is on cuda:{x.device.index}, the resampler on cuda:{self.device}")
        one = x.dim() == 1
        x2 = x.reshape(1, -1) if one else x
        if x2.dim() != 2 or x2.shape[1] < 1 or x2.shape[0] < 1:
            raise GtcrnError(f"x must be (B,L) or (L,) with L >= 1, got {tuple(x.shape)}")
        if x2.stride(1) != 1 and x2.shape[1] > 1:
            x2 = x2.contiguous()
        B, L = x2.shape
        n = self.out_len(L)
        if out is None:
            out2 = torch.empty((B, n), device=x.device, dtype=out_dtype or torch.float32)
        else:
            out2 = out.reshape(1, -1) if (one and out.dim() == 1) else out
            if (not isinstance(out2, torch.Tensor) or out2.device != x.device or out2.dim() != 2 or out2.shape[0] != B
                    or out2.shape[1] < n or (out2.stride(1) != 1 and out2.shape[1] > 1)
                    or out2.dtype not in (torch.float32, torch.int16)):
                raise GtcrnError(f"out must be a float32 or int16 tensor of shape ({B}, >= {n}) with contiguous rows")
        if x2.dtype == torch.int16 and out2.dtype == torch.int16:
            raise GtcrnError("int16 -> int16 is not offered: one side is float32")
        lens = None
        if lengths is not None:
            lens = torch.as_tensor(lengths).reshape(-1)
            if lens.numel() != B:
                raise GtcrnError(f"lengths must hold {B} entries, got {lens.numel()}")
            if not lens.is_cuda:
                if int(lens.min()) < 0 or int(lens.max()) > L:
                    raise GtcrnError(f"every length must lie in [0, L={L}]")
            lens = lens.to(device=x.device, dtype=torch.int32).contiguous()
        fn = (lib().gtcrn_resample_pcm16_in if x2.dtype == torch.int16 else
              lib().gtcrn_resample_pcm16_out if out2.dtype == torch.int16 else lib().gtcrn_resample)
        with torch.cuda.device(x.device):
            # (a one-row tensor may report any stride)
            _check(fn(self._h, x2.data_ptr(), max(x2.stride(0), L), lens.data_ptr() if lens is not None else None, L,
                      out2.data_ptr(), max(out2.stride(0), n), B, _stream_ptr()))
        if out is not None:
            return out
        return out2[0] if one else out2


SCORE_BITS = {"sdr": 1, "sisnr": 2, "stoi": 4}
SCORE_STAGES = 6
SCORE_EXT_BITS = dict(SCORE_BITS, estoi=8, segsnr=16)
SCORE_EXT_SEGS_PER_WG = 8      # ESTOI segments per workgroup (csrc/metrics.h: SX_SEGS_PER_WG), for the tests' edge lengths


def score_taps():
    """(up, down, h) of the scorer's 16 kHz -> 10 kHz stage: 5, 8 and the 513 float32 taps the kernel uses (host only)."""
    up, down = ctypes.c_int(), ctypes.c_int()
    n = _check(lib().gtcrn_score_taps(ctypes.byref(up), ctypes.byref(down), None, 0))
    h = np.empty(n, np.float32)
    _check(lib().gtcrn_score_taps(ctypes.byref(up), ctypes.byref(down), h.ctypes.data_as(_c_f32p), n))
    return up.value, down.value, h


def score_bands():
    """(lo, hi): the 15 third-octave bin ranges lo[j] .. hi[j] - 1 of STOI's envelopes (host only)."""
    lo, hi = (ctypes.c_int * 15)(), (ctypes.c_int * 15)()
    _check(lib().gtcrn_score_bands(lo, hi))
    return list(lo), list(hi)


def score_frames(L):
    """Analysis frames of an L-sample 16 kHz clip at STOI's 10 kHz (host only)."""
    return _check(lib().gtcrn_score_frames(int(L)))


class Scorer:
    """SDR, SI-SNR and STOI of (clean, enhanced) 16 kHz pairs on one device (gtcrn_scorer; "scores" in
    include/gtcrn_micro_hip.h): eval/eval_intrusive_metrics.py's three arithmetic metrics without a copy to the host.
    Not PESQ, not DNSMOS."""

    def __init__(self, device=0):
        self.device = int(device)
        h = ctypes.c_void_p()
        _check(lib().gtcrn_scorer_create(ctypes.byref(h), self.device))
        self._h = h
        self._ws = {}          # (B, L) -> workspace
        self._captured = set()
        self._ws_ext = {}      # the same two for score_ext
        self._captured_ext = set()

    def close(self):
        if getattr(self, "_h", None):
            lib().gtcrn_scorer_destroy(self._h)
            self._h = None
            self._ws = {}
            self._ws_ext = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, B, L):
        n = int(lib().gtcrn_score_workspace_bytes(int(B), int(L)))
        if n == 0:
            raise GtcrnError(lib().gtcrn_last_error().decode())
        return n

    def _rows(self, x, name):
        import torch
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
            raise GtcrnError(f"{name} must be a float32 CUDA (ROCm) tensor")
        if x.device.index != self.device:
            raise GtcrnError(f"{name} is on cuda:{x.device.index}, the scorer on cuda:{self.device}")
        x2 = x.reshape(1, -1) if x.dim() == 1 else x
        if x2.dim() != 2 or x2.shape[0] < 1 or x2.shape[1] < 1:
            raise GtcrnError(f"{name} must be (B,L) or (L,) with L >= 1, got {tuple(x.shape)}")
        if (x2.stride(1) != 1 and x2.shape[1] > 1) or (x2.shape[0] > 1 and x2.stride(0) < x2.shape[1]):
            x2 = x2.contiguous()      # (also a broadcast row, clean.expand(B, L): stride 0 between the rows)
        return x2

    def score(self, ref, inf, lengths=None, what=("sdr", "sisnr", "stoi"), out=None):
        """ref, inf: (B,L) or (L,) float32 CUDA tensors of equal shape, 16 kHz.  lengths (optional, B ints, host or
        device): row b holds lengths[b] <= L samples.  what: names out of "sdr", "sisnr", "stoi".  out (optional): a
        contiguous (B,4) float64 tensor that receives the 32-byte records (for a captured call).  Returns a dict of (B,)
        device tensors: float64 "sdr", "sisnr", "stoi" (0 where not asked for), int32 "kept_frames" and "segments", all
        views of "records".  Asynchronous on the current stream; nothing is copied to the host."""
        import torch
        r2, y2 = self._rows(ref, "ref"), self._rows(inf, "inf")
        if r2.shape != y2.shape:
            raise GtcrnError(f"ref {tuple(ref.shape)} and inf {tuple(inf.shape)} must have one shape")
        B, L = r2.shape
        bits = 0
        for name in ((what,) if isinstance(what, str) else what):
            if name not in SCORE_BITS:
                raise GtcrnError(f"unknown score {name!r}: choose from {sorted(SCORE_BITS)}")
            bits |= SCORE_BITS[name]
        lens = None
        if lengths is not None:
            lens = torch.as_tensor(lengths).reshape(-1)
            if lens.numel() != B:
                raise GtcrnError(f"lengths must hold {B} entries, got {lens.numel()}")
            if not lens.is_cuda and (int(lens.min()) < 0 or int(lens.max()) > L):
                raise GtcrnError(f"every length must lie in [0, L={L}]")
            lens = lens.to(device=r2.device, dtype=torch.int32).contiguous()
        if out is None:
            rec = torch.empty((B, 4), device=r2.device, dtype=torch.float64)
        else:
            rec = out
            if (not isinstance(rec, torch.Tensor) or rec.device != r2.device or rec.dtype != torch.float64
                    or tuple(rec.shape) != (B, 4) or not rec.is_contiguous()):
                raise GtcrnError(f"out must be a contiguous float64 tensor of shape ({B}, 4) on the inputs' device")
        ws = None
        if bits & 4:
            ws = self._ws.get((B, L))
            if ws is None:
                free = [k for k in self._ws if k not in self._captured]
                if len(free) >= 8:          # a folder of many lengths: keep the eight most recent shapes
                    self._ws.pop(free[0])
                ws = self._ws[(B, L)] = torch.empty(self.workspace_bytes(B, L), device=r2.device, dtype=torch.uint8)
        if ws is not None and torch.cuda.is_current_stream_capturing():
            self._captured.add((B, L))      # a graph holds this workspace's address: never dropped
        with torch.cuda.device(r2.device):
            # (a one-row tensor may report any stride)
            _check(lib().gtcrn_score(self._h, r2.data_ptr(), max(r2.stride(0), L), y2.data_ptr(), max(y2.stride(0), L),
                                     lens.data_ptr() if lens is not None else None, L, B, bits, rec.data_ptr(),
                                     ws.data_ptr() if ws is not None else None, _stream_ptr()))
        self._last_L = L
        counts = rec.view(torch.int32)[:, 6:8]
        return {"sdr": rec[:, 0], "sisnr": rec[:, 1], "stoi": rec[:, 2], "kept_frames": counts[:, 0],
                "segments": counts[:, 1], "records": rec}

    def ext_workspace_bytes(self, B, L):
        n = int(lib().gtcrn_score_ext_workspace_bytes(int(B), int(L)))
        if n == 0:
            raise GtcrnError(lib().gtcrn_last_error().decode())
        return n

    def score_ext(self, ref, inf, lengths=None, what=("sdr", "sisnr", "stoi", "estoi", "segsnr"), out=None):
        """score() with ESTOI and segmental SNR (gtcrn_score_ext; "scores, extended" in include/gtcrn_micro_hip.h).  Same
        ref, inf and lengths.  what: names out of "sdr", "sisnr", "stoi", "estoi", "segsnr".  out (optional): a contiguous
        (B,8) float64 tensor that receives the 64-byte records.  Returns score()'s keys plus float64 "estoi", "segsnr" and
        int32 "segsnr_frames", all views of "records"; with what out of score()'s three, columns 0 .. 3 are score()'s
        record bit for bit and the rest is 0.  Asynchronous on the current stream; nothing is copied to the host."""
        import torch
        r2, y2 = self._rows(ref, "ref"), self._rows(inf, "inf")
        if r2.shape != y2.shape:
            raise GtcrnError(f"ref {tuple(ref.shape)} and inf {tuple(inf.shape)} must have one shape")
        B, L = r2.shape
        bits = 0
        for name in ((what,) if isinstance(what, str) else what):
            if name not in SCORE_EXT_BITS:
                raise GtcrnError(f"unknown score {name!r}: choose from {sorted(SCORE_EXT_BITS)}")
            bits |= SCORE_EXT_BITS[name]
        lens = None
        if lengths is not None:
            lens = torch.as_tensor(lengths).reshape(-1)
            if lens.numel() != B:
                raise GtcrnError(f"lengths must hold {B} entries, got {lens.numel()}")
            if not lens.is_cuda and (int(lens.min()) < 0 or int(lens.max()) > L):
                raise GtcrnError(f"every length must lie in [0, L={L}]")
            lens = lens.to(device=r2.device, dtype=torch.int32).contiguous()
        if out is None:
            rec = torch.empty((B, 8), device=r2.device, dtype=torch.float64)
        else:
            rec = out
            if (not isinstance(rec, torch.Tensor) or rec.device != r2.device or rec.dtype != torch.float64
                    or tuple(rec.shape) != (B, 8) or not rec.is_contiguous()):
                raise GtcrnError(f"out must be a contiguous float64 tensor of shape ({B}, 8) on the inputs' device")
        ws = None
        if bits & 28:
            ws = self._ws_ext.get((B, L))
            if ws is None:
                free = [k for k in self._ws_ext if k not in self._captured_ext]
                if len(free) >= 8:          # as score(): keep the eight most recent shapes
                    self._ws_ext.pop(free[0])
                ws = self._ws_ext[(B, L)] = torch.empty(self.ext_workspace_bytes(B, L), device=r2.device, dtype=torch.uint8)
        if ws is not None and torch.cuda.is_current_stream_capturing():
            self._captured_ext.add((B, L))  # a graph holds this workspace's address: never dropped
        with torch.cuda.device(r2.device):
            _check(lib().gtcrn_score_ext(self._h, r2.data_ptr(), max(r2.stride(0), L), y2.data_ptr(), max(y2.stride(0), L),
                                         lens.data_ptr() if lens is not None else None, L, B, bits, rec.data_ptr(),
                                         ws.data_ptr() if ws is not None else None, _stream_ptr()))
        ints = rec.view(torch.int32)
        return {"sdr": rec[:, 0], "sisnr": rec[:, 1], "stoi": rec[:, 2], "kept_frames": ints[:, 6], "segments": ints[:, 7],
                "estoi": rec[:, 4], "segsnr": rec[:, 5], "segsnr_frames": ints[:, 12], "records": rec}

    def debug(self, which, b=0):
        """Test hook (gtcrn_score_debug; synchronises): one intermediate of row b of the most recent call with STOI as a
        float32 tensor: 0 the 10 kHz ref, 1 frame energies in dB, 2 the keep mask, 3 / 4 the ref / inf envelopes (15, M)."""
        import torch
        L = getattr(self, "_last_L", 1)
        cap = max(L, 15 * (score_frames(L) + 1))
        dst = torch.empty(cap, device=f"cuda:{self.device}", dtype=torch.float32)
        with torch.cuda.device(self.device):
            n = _check(lib().gtcrn_score_debug(self._h, int(which), int(b), dst.data_ptr(), cap, _stream_ptr()))
        got = dst[:n].clone()
        return got.reshape(15, n // 15) if which in (3, 4) else got

    def timing(self, on=True):
        _check(lib().gtcrn_score_timing(self._h, 1 if on else 0))

    def timing_read(self):
        """{launch name: milliseconds} of the most recent call made with timing on (synchronises on its last event)."""
        res = {}
        for i in range(SCORE_STAGES):
            name, ms = ctypes.create_string_buffer(64), ctypes.c_float()
            _check(lib().gtcrn_score_timing_read(self._h, i, name, 64, ctypes.byref(ms)))
            res[name.value.decode()] = float(ms.value)
        return res

    def ext_timing_read(self):
        """timing_read() for the most recent score_ext (gtcrn_score_ext_timing_read; timing(True) arms both)."""
        res = {}
        for i in range(lib().gtcrn_score_ext_stages()):
            name, ms = ctypes.create_string_buffer(64), ctypes.c_float()
            _check(lib().gtcrn_score_ext_timing_read(self._h, i, name, 64, ctypes.byref(ms)))
            res[name.value.decode()] = float(ms.value)
        return res


G711_LAWS = {"ulaw": 0, "alaw": 1}


def g711_law(law):
    """"ulaw" / "alaw" (or 0 / 1) -> the C ABI's law number; None stays None (no G.711)."""
    if law is None:
        return None
    if isinstance(law, str) and law in G711_LAWS:
        return G711_LAWS[law]
    if not isinstance(law, (str, bool)) and law in (0, 1):
        return int(law)
    raise GtcrnError(f'g711 must be "ulaw", "alaw" or None, got {law!r}')


def _need_law(law, who):
    law = g711_law(law)
    if law is None:
        raise GtcrnError(f'{who}: law must be "ulaw" or "alaw"')
    return law


def _g711_rows(state, x, what):
    """uint8 rows are G.711 codes and need the law the state was made with: refused here, before any library call."""
    import torch
    if isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and getattr(state, "g711", None) is None:
        raise GtcrnError(f'{what} is uint8 (G.711 codes) but the state was made without a law: pass g711="ulaw" or "alaw" '
                         "to new_packet_state / new_packet_slot_state")


def g711_decode_table(law):
    """D_law as a numpy int16 array of 256 entries: code c is the sample D_law[c] / 32768 (host only)."""
    import numpy as np
    tab = np.empty(256, dtype=np.int16)
    _check(lib().gtcrn_g711_decode_table(_need_law(law, "g711_decode_table"), tab.ctypes.data_as(ctypes.POINTER(ctypes.c_short))))
    return tab


def g711_encode_pcm16(law, p):
    """E_law(p): the code of the int16 value p (host only; raises for p outside -32768 .. 32767)."""
    return _check(lib().gtcrn_g711_encode_pcm16(_need_law(law, "g711_encode_pcm16"), int(p)))


def _g711_pair(codes, wave, who):
    import torch
    for t, dt, what in ((codes, torch.uint8, "uint8"), (wave, torch.float32, "float32")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise GtcrnError(f"{who}: a contiguous {what} CUDA tensor is required")
    if codes.numel() != wave.numel() or codes.device != wave.device:
        raise GtcrnError(f"{who}: the two tensors must hold the same number of samples on one device")
    if codes.numel() % 16 or codes.data_ptr() % 16 or wave.data_ptr() % 16:
        raise GtcrnError(f"{who}: 16-byte aligned tensors, a sample count that is a multiple of 16")


def g711_to_f32(codes, law, out=None):
    """G.711 codes (uint8) -> float32 waveform on the device, x = D_law[c] / 32768 (exact); asynchronous on the current
    stream of the tensor's device (gtcrn_g711_to_f32).  For the offline and hop-form caller."""
    import torch
    law = _need_law(law, "g711_to_f32")
    if out is None:
        out = torch.empty(codes.shape, dtype=torch.float32, device=codes.device)
    _g711_pair(codes, out, "g711_to_f32")
    with torch.cuda.device(codes.device):
        _check(lib().gtcrn_g711_to_f32(codes.device.index, law, ctypes.c_void_p(codes.data_ptr()),
                                       ctypes.c_void_p(out.data_ptr()), int(codes.numel()), _stream_ptr()))
    return out


def f32_to_g711(wave, law, out=None):
    """float32 waveform -> G.711 codes (uint8) on the device: E_law(clip(rint(y * 32768), -32768, 32767)), i.e. f32_to_pcm16
    and then the integer map; asynchronous on the current stream of the tensor's device (gtcrn_f32_to_g711)."""
    import torch
    law = _need_law(law, "f32_to_g711")
    if out is None:
        out = torch.empty(wave.shape, dtype=torch.uint8, device=wave.device)
    _g711_pair(out, wave, "f32_to_g711")
    with torch.cuda.device(wave.device):
        _check(lib().gtcrn_f32_to_g711(wave.device.index, law, ctypes.c_void_p(wave.data_ptr()),
                                       ctypes.c_void_p(out.data_ptr()), int(wave.numel()), _stream_ptr()))
    return out


def _pcm_pair(pcm, wave, who):
    import torch
    for t, dt, what in ((pcm, torch.int16, "int16"), (wave, torch.float32, "float32")):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise GtcrnError(f"{who}: a contiguous {what} CUDA tensor is required")
    if pcm.numel() != wave.numel() or pcm.device != wave.device:
        raise GtcrnError(f"{who}: the two tensors must hold the same number of samples on one device")
    if pcm.numel() % 8 or pcm.data_ptr() % 16 or wave.data_ptr() % 16:
        raise GtcrnError(f"{who}: 16-byte aligned tensors, a sample count that is a multiple of 8")


def pcm16_to_f32(pcm, out=None):
    """int16 samples -> float32 waveform on the device (x = s / 32768, exact: what soundfile.read returns, infer.py:54);
    asynchronous on the current stream of the tensor's device (gtcrn_pcm16_to_f32)."""
    import torch
    if out is None:
        out = torch.empty(pcm.shape, dtype=torch.float32, device=pcm.device)
    _pcm_pair(pcm, out, "pcm16_to_f32")
    with torch.cuda.device(pcm.device):
        _check(lib().gtcrn_pcm16_to_f32(pcm.device.index, ctypes.c_void_p(pcm.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                        int(pcm.numel()), _stream_ptr()))
    return out


def f32_to_pcm16(wave, out=None):
    """float32 waveform -> int16 samples on the device: clip(rint(y * 32768), -32768, 32767), round half to even (the
    16-bit PCM sf.write / scipy.io.wavfile.write of np.rint produce, infer.py:113); asynchronous on the current stream of
    the tensor's device (gtcrn_f32_to_pcm16)."""
    import torch
    if out is None:
        out = torch.empty(wave.shape, dtype=torch.int16, device=wave.device)
    _pcm_pair(out, wave, "f32_to_pcm16")
    with torch.cuda.device(wave.device):
        _check(lib().gtcrn_f32_to_pcm16(wave.device.index, ctypes.c_void_p(wave.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                        int(wave.numel()), _stream_ptr()))
    return out


def stream_streams_per_workgroup(nstreams):
    """Streams per workgroup (4: k_stream_ms, 7: k_stream_wide) of the one-launch step the library picks for `nstreams`
    single-frame steps (host logic only)."""
    return _check(lib().gtcrn_stream_streams_per_workgroup(int(nstreams)))


def selftest_mfma(device=0):
    _check(lib().gtcrn_selftest_mfma(int(device)))


def selftest_mfma_i8(device=0):
    """The lane maps of v_mfma_i32_16x16x64_i8 that the reverb convolution's matrix form relies on (exact integer data)."""
    _check(lib().gtcrn_selftest_mfma_i8(int(device)))


def selftest_split3(x, A=None, B=None, device=0):
    """Device-side split3 / join3 / split_mm6 (the dense 3x3's exact bf16 split) on the given fp32 values: returns
    (planes (3,n), joined (n,)) and, with A (16,32) and B (32,16), also D (16,16) = A @ B through the six products."""
    x = np.ascontiguousarray(x, np.float32).ravel()
    planes = np.empty((3, x.size), np.float32)
    joined = np.empty(x.size, np.float32)
    f = lambda a: a.ctypes.data_as(_c_f32p)
    if A is None:
        _check(lib().gtcrn_selftest_split3(int(device), f(x), x.size, f(planes), f(joined), None, None, None))
        return planes, joined
    A = np.ascontiguousarray(A, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    assert A.shape == (16, 32) and B.shape == (32, 16)
    D = np.empty((16, 16), np.float32)
    _check(lib().gtcrn_selftest_split3(int(device), f(x), x.size, f(planes), f(joined), f(A), f(B), f(D)))
    return planes, joined, D


class Trainer:
    """Train-mode forward/backward of the model on one device (gtcrn_trainer): batch-statistics
    BatchNorm, saved activations, gradients of the 248 trainable tensors in the canonical blob layout."""

    def __init__(self, device=0):
        self.device = int(device)
        h = ctypes.c_void_p()
        _check(lib().gtcrn_trainer_create(ctypes.byref(h), self.device))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().gtcrn_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # "bf16_saves": what the backward re-reads is stored in bf16 (as in "bf16") while the forward chain itself stays fp32
    # -- the forward is the fp32 network's, bit for bit; the gradient differs only by the rounding of the saved tensors
    # "bf16_grads": "bf16" with the gradients handed between units stored in bf16 too (what bf16 autocast training keeps)
    STORAGE = {"f32": 0, "fp32": 0, "bf16": 1, "bf16_saves": 4, "bf16_grads": 5}

    @staticmethod
    def workspace_bytes(B, T, storage="f32"):
        return int(lib().gtcrn_train_workspace_bytes2(int(B), int(T), Trainer.STORAGE[storage]))

    def set_storage(self, storage):
        """Storage of the saved activations: "f32" (the reference's precision), "bf16" (BASELINE configs[3]: bf16
        activations in the forward too), "bf16_saves" (bf16 copies for the backward only, fp32 forward chain) or
        "bf16_grads" ("bf16" whose inter-unit gradient tensors are bf16 as well); arithmetic, statistics, parameter
        gradients and weights are fp32 in all of them."""
        if storage not in self.STORAGE:
            raise GtcrnError(f"storage must be one of {sorted(self.STORAGE)}, got {storage!r}")
        _check(lib().gtcrn_trainer_set_storage(self._h, self.STORAGE[storage]))
        self.storage = storage

    def planned_workspace_bytes(self, B, T):
        """Workspace of a (B, T) problem with THIS trainer's storage mode and fusion mask (the static
        ``workspace_bytes`` describes the default mask only)."""
        return int(_check(lib().gtcrn_trainer_workspace_bytes(self._h, int(B), int(T))))

    def set_fusions(self, mask):
        """Diagnostic (gtcrn_trainer_set_fusions): 65535 = all pass fusions (default), 32767 = the weight-gradient finishes launched one by one, 16383 = the TCN's dilated depthwise forward through the general kernel, 8191 = the pointwise forward convs through the general conv kernel too, 4095 = without point_bn2 on load, 2047 =
        also without the producer-written decoder sums, 1023 = also without the in-launch finish of the BatchNorm reductions (round 4's), 7 = round 3's (every activation stored, separate skip-gradient adds),
        0 = the layer-at-a-time passes."""
        _check(lib().gtcrn_trainer_set_fusions(self._h, int(mask)))

    def _check_blob(self, blob, what):
        _require_cuda_f32(blob, what)
        if blob.numel() != NPARAM_FLOATS or not blob.is_contiguous():
            raise GtcrnError(f"{what} must be a contiguous tensor of {NPARAM_FLOATS} floats")

    def forward(self, params, spec, out=None):
        """params: canonical blob on the device (running statistics are updated in place); spec (B,257,T,2)."""
        import torch
        self._check_blob(params, "params")
        _require_cuda_f32(spec, "spec")
        if spec.dim() != 4 or spec.shape[1] != NBINS or spec.shape[3] != 2:
            raise GtcrnError(f"spec must be (B,257,T,2), got {tuple(spec.shape)}")
        if spec.stride(3) != 1:
            spec = spec.contiguous()
        B, _, T, _ = spec.shape
        if out is None:
            out = _empty_spec_like(spec)
        isb, isf, ist = _spec_strides(spec)
        osb, osf, ost = _spec_strides(out)
        with torch.cuda.device(self.device):
            _check(lib().gtcrn_train_forward(self._h, params.data_ptr(), spec.data_ptr(), isb, isf, ist,
                                             out.data_ptr(), osb, osf, ost, B, T, _stream_ptr()))
        return out

    def backward(self, params, spec, grad_out, grads=None):
        """Gradients (canonical blob layout) of the most recent forward for the upstream gradient grad_out."""
        import torch
        self._check_blob(params, "params")
        _require_cuda_f32(grad_out, "grad_out")
        if spec.stride(3) != 1:
            spec = spec.contiguous()
        if grad_out.stride(3) != 1:
            grad_out = grad_out.contiguous()
        if grads is None:
            grads = torch.empty(NPARAM_FLOATS, device=params.device, dtype=torch.float32)
        self._check_blob(grads, "grads")
        isb, isf, ist = _spec_strides(spec)
        gsb, gsf, gst = _spec_strides(grad_out)
        with torch.cuda.device(self.device):
            _check(lib().gtcrn_train_backward(self._h, params.data_ptr(), spec.data_ptr(), isb, isf, ist,
                                              grad_out.data_ptr(), gsb, gsf, gst, grads.data_ptr(), _stream_ptr()))
        return grads

    def hybrid_loss(self, pred, true, want_grad=True):
        """HybridLoss (loss.py:30-71) of two (B,257,T,2) spectrograms: returns (loss 0-d tensor, d loss/d pred or None)."""
        import torch
        _require_cuda_f32(pred, "pred")
        _require_cuda_f32(true, "true")
        if pred.shape != true.shape or pred.dim() != 4 or pred.shape[1] != NBINS or pred.shape[3] != 2:
            raise GtcrnError(f"pred/true must both be (B,257,T,2), got {tuple(pred.shape)} and {tuple(true.shape)}")
        if pred.stride(3) != 1:
            pred = pred.contiguous()
        if true.stride(3) != 1:
            true = true.contiguous()
        B, _, T, _ = pred.shape
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        grad = _empty_spec_like(pred) if want_grad else None      # (the gradient takes pred's memory order)
        psb, psf, pst = _spec_strides(pred)
        tsb, tsf, tst = _spec_strides(true)
        gsb, gsf, gst = _spec_strides(grad) if want_grad else (0, 0, 0)
        with torch.cuda.device(self.device):
            _check(lib().gtcrn_train_loss_strided(self._h, pred.data_ptr(), psb, psf, pst, true.data_ptr(), tsb, tsf, tst,
                                                  B, T, loss.data_ptr(), grad.data_ptr() if want_grad else None,
                                                  gsb, gsf, gst, _stream_ptr()))
        self._loss_B = B
        return loss, grad

    def hybrid_loss_terms(self):
        """Test hook: the per-utterance SI-SNR terms (float64 numpy, (B,)) of the most recent hybrid_loss call on this
        trainer, read before any other call on it (gtcrn_train_loss_terms)."""
        import torch
        B = getattr(self, "_loss_B", 0)
        if B < 1:
            raise GtcrnError("hybrid_loss_terms: no hybrid_loss call on this trainer yet")
        out = np.empty(B, np.float64)
        with torch.cuda.device(self.device):
            _check(lib().gtcrn_train_loss_terms(self._h, out.ctypes.data_as(_vp), B, _stream_ptr()))
        return out

    def tap(self, name):
        """A tensor the most recent forward stored, as (B,C,T,F) float32: a stage boundary (en0..en4, tcn0..tcn7,
        gtcn1, gtcn2, de0..de4), a decoder sum (sum0..sum4, where stored) or a unit's stored conv output
        "<BatchNorm prefix>.y" (bf16 modes: the centred bf16 copy, no shift added back).  See gtcrn_train_tap."""
        import torch
        sh = (ctypes.c_long * 4)()
        _check(lib().gtcrn_train_tap(self._h, name.encode(), None, sh, None))
        out = torch.empty(tuple(sh), device=f"cuda:{self.device}", dtype=torch.float32)
        with torch.cuda.device(self.device):
            _check(lib().gtcrn_train_tap(self._h, name.encode(), out.data_ptr(), sh, _stream_ptr()))
        return out.permute(0, 3, 1, 2).contiguous()


_adam_ws = {}


def clip_adam_workspace(device, n=None):
    """A zeroed workspace for clip_adam_step (ticket + partial sums; every call leaves the ticket at zero again).  One per
    caller that may step concurrently with another on the same device (FlatAdam owns one per instance)."""
    import torch
    n = NPARAM_FLOATS if n is None else n
    return torch.zeros((int(lib().gtcrn_clip_adam_workspace_bytes(n)) + 7) // 8, dtype=torch.float64, device=device)


def clip_adam_step(params, grads, exp_avg, exp_avg_sq, mask, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                   max_norm=0.0, norm_out=None, ws=None):
    """clip_grad_norm_(max_norm) + torch.optim.Adam.step() over flat fp32 device blobs in two launches
    (gtcrn_clip_adam_step).  norm_out: optional 2-float device tensor (total norm, clip coefficient).  ws: the caller's own
    workspace (clip_adam_workspace); without one a per-(device, size) workspace shared by such callers is used -- fine for
    one stream per device."""
    import torch
    n = params.numel()
    for t, what in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (mask, "mask")):
        _require_cuda_f32(t, what)
        if t.numel() != n or not t.is_contiguous() or t.device != params.device:
            raise GtcrnError(f"{what} must be a contiguous float32 tensor of {n} elements on {params.device}")
    if norm_out is not None:
        _require_cuda_f32(norm_out, "norm_out")
        if norm_out.numel() < 2 or not norm_out.is_contiguous():
            raise GtcrnError("norm_out must hold 2 contiguous floats")
    if ws is None:
        key = (params.device.index, n)
        ws = _adam_ws.get(key)
        if ws is None:      # zeroed once: every call leaves the ticket at zero again
            ws = _adam_ws[key] = clip_adam_workspace(params.device, n)
    elif ws.device != params.device or ws.numel() * ws.element_size() < int(lib().gtcrn_clip_adam_workspace_bytes(n)):
        raise GtcrnError("clip_adam_step: the workspace is on another device or too small")
    with torch.cuda.device(params.device):
        _check(lib().gtcrn_clip_adam_step(params.device.index, params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(),
                                          exp_avg_sq.data_ptr(), mask.data_ptr(), n, float(max_norm), float(lr),
                                          float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step),
                                          norm_out.data_ptr() if norm_out is not None else None, ws.data_ptr(),
                                          _stream_ptr()))
