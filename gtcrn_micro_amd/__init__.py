"""gtcrn_micro_amd -- MI355X (gfx950) native hot path of GTCRN-Micro.

Layout mirrors the reference package for the path it replaces:
  gtcrn_micro_amd.models.gtcrn_micro.GTCRNMicro               <- gtcrn_micro.models.gtcrn_micro.GTCRNMicro
  gtcrn_micro_amd.streaming.gtcrn_micro_stream.StreamGTCRNMicro <- gtcrn_micro.streaming.gtcrn_micro_stream
  gtcrn_micro_amd.streaming.conversion.convert.convert_to_stream
The arithmetic lives in csrc/ (HIP, built into libgtcrn_micro_hip.so) behind the C ABI of
include/gtcrn_micro_hip.h; nothing here falls back to the CPU.
"""
from ._lib import tone_params, tone_table, tone_block, f32_to_pcm16, pcm16_to_f32, Engine, GtcrnError, Trainer, istft, make_window, num_frames, selftest_mfma, selftest_mfma_i8, selftest_split3, stft, stft_frames, WaveStreamState, RateStreamState, PacketStreamState, PacketSlotState, Resampler, resample_taps, packet_stream_n16, packet_stream_latency16, atten_lim_to_gain, gain_ramp, alc_params, alc_block, level_dbov, g711_to_f32, f32_to_g711, g711_decode_table, g711_encode_pcm16, Scorer, score_taps, score_bands, score_frames  # noqa: F401
from . import data  # noqa: F401
from .data import BatchSource, Corpus, RirBank  # noqa: F401
from . import mixer  # noqa: F401
from .mixer import Mixer, mix_params, mix_rooms_host  # noqa: F401
from . import plc  # noqa: F401
from .plc import Concealer, plc_params, plc_rows_host  # noqa: F401

__all__ = ["alc_params", "alc_block", "tone_params", "tone_table", "tone_block", "pcm16_to_f32", "f32_to_pcm16", "Engine", "GtcrnError", "Trainer", "stft", "istft", "stft_frames", "make_window", "num_frames", "selftest_mfma", "selftest_split3", "WaveStreamState", "RateStreamState", "PacketStreamState", "PacketSlotState", "Resampler", "resample_taps", "packet_stream_n16", "packet_stream_latency16", "atten_lim_to_gain", "gain_ramp", "level_dbov", "g711_to_f32", "f32_to_g711", "g711_decode_table", "g711_encode_pcm16", "Scorer", "score_taps", "score_bands", "score_frames", "data", "Corpus", "BatchSource", "mixer", "Mixer", "mix_params", "mix_rooms_host", "plc", "Concealer", "plc_params", "plc_rows_host"]
