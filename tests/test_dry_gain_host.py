"""CPU-side checks of the attenuation limit (the *_limited calls, include/gtcrn_micro_hip.h "attenuation limit"): the ABI,
the dB -> dry gain convention, the argument checks that answer before the device is touched, and the properties of the
mixing formula that the GPU tests lean on, in numpy float32."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft

LIMITED_SYMBOLS = ["gtcrn_forward_wave_limited", "gtcrn_wave_stream_step_limited", "gtcrn_wave_stream_step_limited_pcm16",
                   "gtcrn_wave_stream_flush_limited", "gtcrn_wave_stream_flush_limited_pcm16",
                   "gtcrn_rate_stream_step_limited", "gtcrn_rate_stream_step_limited_pcm16",
                   "gtcrn_packet_stream_set_dry_gain"]
ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def mix(beta, x, w):
    """The contract's formula: four float32 roundings, no fused multiply-add."""
    beta, x, w = np.float32(beta), np.asarray(x, np.float32), np.asarray(w, np.float32)
    return (beta * x).astype(np.float32) + ((np.float32(1) - beta) * w).astype(np.float32)


def test_limited_symbols_exported_and_declared():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    with open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")) as f:
        header = f.read()
    for n in LIMITED_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n


def test_abi_version_and_state_sizes_unchanged():
    """The limit adds no state: every *_state_bytes is what it was, and so is the ABI version."""
    from gtcrn_micro_amd import _lib
    L = _lib.lib()
    assert L.gtcrn_abi_version() == 1
    assert L.gtcrn_stream_state_bytes() == 4 * 38116
    assert L.gtcrn_wave_stream_state_bytes() == 4 * (512 + 256 + 4)
    # the filter histories of the rate form (the formulas of tests/test_packet_host.py: ntp per stage)
    import resample_checker as RC
    ntp = lambda half, up: (2 * half // up + 1 + 3) // 4 * 4
    for fs in (8000, 24000, 32000, 48000):
        up, _, half, _ = RC.design(fs, 16000)
        upo, _, halfo, _ = RC.design(16000, fs)
        assert _lib.rate_stream_state_bytes(fs) == 4 * (ntp(half, up) + ntp(halfo, upo)), fs
        assert _lib.packet_stream_state_bytes(fs, fs // 100) == 4 * (512 + ntp(half, up) + ntp(halfo, upo)), fs
    assert _lib.packet_stream_state_bytes(16000, 160) == 4 * 512


def test_atten_lim_to_gain():
    from gtcrn_micro_amd import atten_lim_to_gain
    assert atten_lim_to_gain(None) == 0.0
    assert atten_lim_to_gain(float("inf")) == 0.0
    assert atten_lim_to_gain(0) == 1.0 and atten_lim_to_gain(0.0) == 1.0
    for db in (6, 12, 20, 3.5):
        assert atten_lim_to_gain(db) == 10.0 ** (-db / 20.0)
        assert 0.0 < atten_lim_to_gain(db) < 1.0
    assert math.isclose(atten_lim_to_gain(20), 0.1)
    for bad in (-1, -1e-9, float("nan"), -float("inf")):
        with pytest.raises(ValueError):
            atten_lim_to_gain(bad)


def test_null_arguments_are_argument_errors_before_the_device():
    from gtcrn_micro_amd._lib import lib
    L = lib()
    p = ctypes.c_void_p(16)           # never dereferenced: every call below is rejected before the device is touched
    calls = [
        lambda: L.gtcrn_wave_stream_step_limited(None, p, p, p, 256, p, 256, 1, 1, p, p, None),
        lambda: L.gtcrn_wave_stream_step_limited_pcm16(None, p, p, p, 256, p, 256, 1, 1, p, p, None),
        lambda: L.gtcrn_wave_stream_flush_limited(None, p, p, p, 256, 10, p, 256, 1, p, p, None),
        lambda: L.gtcrn_wave_stream_flush_limited_pcm16(None, p, p, p, 256, 10, p, 256, 1, p, p, None),
        lambda: L.gtcrn_rate_stream_step_limited(None, p, p, p, p, p, p, 768, p, 768, 1, 1, p, p, None),
        lambda: L.gtcrn_rate_stream_step_limited_pcm16(None, p, p, p, p, p, p, 768, p, 768, 1, 1, p, p, None),
        lambda: L.gtcrn_rate_stream_step_limited(p, None, None, p, p, p, p, 768, p, 768, 1, 1, p, p, None),
        lambda: L.gtcrn_packet_stream_set_dry_gain(None, p),
        lambda: L.gtcrn_packet_stream_set_dry_gain(None, None),
    ]
    for i, c in enumerate(calls):
        assert c() == ERR_ARG, i
        assert b"null" in L.gtcrn_last_error(), i


def test_python_layer_rejects_gains_outside_the_unit_interval():
    """Engine._dry_gain is host logic for a float: no device is needed to be told that 1.5 is no gain."""
    from gtcrn_micro_amd import Engine, GtcrnError
    from gtcrn_micro_amd._lib import _gains_of
    eng = Engine.__new__(Engine)                  # no model: only the argument check runs
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(GtcrnError):
            eng._dry_gain(bad, 3, None)
    assert eng._dry_gain(None, 3, None) is None
    g = _gains_of([None, 0, 6], 3)
    assert g.dtype == np.float32 and g[0] == 0.0 and g[1] == 1.0 and g[2] == np.float32(10.0 ** -0.3)
    with pytest.raises(GtcrnError):
        _gains_of([6, 6], 3)
    with pytest.raises(ValueError):
        _gains_of([6, -1, 6], 3)


def test_formula_is_exact_at_both_ends_and_bounded_between():
    """beta = 0 gives w and beta = 1 gives x as values for finite operands; for 0 <= beta <= 1 the mix stays within half
    an ulp-scale of the exact convex combination (each of the four roundings is relative 2^-24)."""
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.standard_normal(4096), [0.0, -0.0, 1e-30, -3e38, 3e38]]).astype(np.float32)
    w = np.concatenate([rng.standard_normal(4096) * 0.1, [-0.0, 0.0, -1e-30, 3e38, -3e38]]).astype(np.float32)
    assert np.array_equal(mix(0.0, x, w), w)
    assert np.array_equal(mix(1.0, x, w), x)
    for db in (6, 12, 3.3):
        b = np.float32(10.0 ** (-db / 20.0))
        got = mix(b, x[:4096], w[:4096]).astype(np.float64)
        exact = float(b) * x[:4096].astype(np.float64) + (1.0 - float(b)) * w[:4096].astype(np.float64)
        bound = 2.0 ** -23 * (np.abs(float(b) * x[:4096]) + np.abs((1.0 - float(b)) * w[:4096])) + 1e-45
        assert np.all(np.abs(got - exact) <= 2 * bound)
