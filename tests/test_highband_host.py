"""CPU-side checks of the high band (gtcrn_rate_stream_step_hb / gtcrn_resample_hb, include/gtcrn_micro_hip.h "high band"):
the symbols and their declarations, the size of the new state and the sizes the feature must leave alone, the argument
errors that are returned without a device, and the checker of the live contract (tests/highband_checker.py) on the case the
contract makes exact."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import highband_checker as HC
import resample_checker as RC

HB_SYMBOLS = ["gtcrn_rate_stream_hb_state_bytes", "gtcrn_rate_stream_hb_reset", "gtcrn_rate_stream_step_hb",
              "gtcrn_rate_stream_step_hb_pcm16", "gtcrn_resample_hb"]
HB_RATES = (24000, 32000, 48000)
ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


@pytest.fixture(scope="module")
def L():
    from gtcrn_micro_amd._lib import lib
    return lib()


def test_symbols_exported_and_declared():
    raw = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    with open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")) as f:
        header = f.read()
    for n in HB_SYMBOLS:
        assert hasattr(raw, n), n
        assert n + "(" in header, n
    assert raw.gtcrn_abi_version() == 1


def test_state_sizes(L):
    """4 (256 + latency) bytes per stream at the three rates, a multiple of 16; no high band elsewhere; the rate state is
    what it was."""
    from gtcrn_micro_amd import _lib
    for fs, lat in ((24000, 480), (32000, 640), (48000, 960)):
        assert _lib.rate_stream_latency(fs) == lat
        assert L.gtcrn_rate_stream_hb_state_bytes(fs) == 4 * (256 + lat)
        assert _lib.rate_stream_hb_state_bytes(fs) == 4 * (256 + lat)
        assert L.gtcrn_rate_stream_hb_state_bytes(fs) % 16 == 0
    for fs in (8000, 16000, 44100, 22050, 11025, 0, 12345):
        assert L.gtcrn_rate_stream_hb_state_bytes(fs) == 0, fs
        assert b"high band" in L.gtcrn_last_error(), fs
        assert L.gtcrn_rate_stream_hb_reset(fs, ctypes.c_void_p(16), 1, None) == ERR_ARG, fs
        with pytest.raises(_lib.GtcrnError):
            _lib.rate_stream_hb_state_bytes(fs)
    for fs in (8000,) + HB_RATES:
        up, down = RC.ratio(fs, 16000)
        nt_in, nt_out = 64 * max(up, down) // up + 1, 64 * max(up, down) // down + 1
        assert _lib.rate_stream_state_bytes(fs) == 4 * ((nt_in + 3) // 4 * 4 + (nt_out + 3) // 4 * 4), fs


def test_argument_errors_are_returned_without_a_device(L):
    p = ctypes.c_void_p(16)           # never dereferenced: every call below is rejected before the device is touched
    calls = [
        lambda: L.gtcrn_rate_stream_step_hb(None, p, p, p, p, p, p, 768, p, 768, 1, 1, None, p, p, p, None),
        lambda: L.gtcrn_rate_stream_step_hb_pcm16(None, p, p, p, p, p, p, 768, p, 768, 1, 1, None, p, p, p, None),
        lambda: L.gtcrn_rate_stream_step_hb(p, None, p, p, p, p, p, 768, p, 768, 1, 1, None, p, p, p, None),
        lambda: L.gtcrn_rate_stream_step_hb(p, p, None, p, p, p, p, 768, p, 768, 1, 1, None, p, p, p, None),
        lambda: L.gtcrn_resample_hb(None, p, 256, p, 256, None, 256, p, 768, None, 768, p, p, 768, 1, None),
        lambda: L.gtcrn_rate_stream_hb_reset(48000, None, 1, None),
        lambda: L.gtcrn_rate_stream_hb_reset(48000, p, 0, None),
        lambda: L.gtcrn_rate_stream_hb_reset(48000, ctypes.c_void_p(20), 1, None),      # off the 16-byte grid
        lambda: L.gtcrn_rate_stream_hb_reset(8000, p, 1, None),
        lambda: L.gtcrn_rate_stream_hb_reset(44100, p, 1, None),
    ]
    for i, c in enumerate(calls):
        assert c() == ERR_ARG, i
        assert L.gtcrn_last_error(), i


@pytest.mark.parametrize("fs", HB_RATES)
def test_checker_bypass_is_exact(fs):
    """w = a one hop late (what the attenuation limit at 0 dB guarantees) and gamma = 1: s == 0, v == 0 and the checker
    returns x delayed by LAT exactly, with a bound of two roundings of x alone."""
    from gtcrn_micro_amd._lib import resample_taps, rate_stream_latency, rate_stream_hop
    up, down, h = resample_taps(16000, fs)
    H, K = rate_stream_hop(fs), 5
    rng = np.random.default_rng(fs)
    a = rng.standard_normal(256 * K).astype(np.float32)
    x = rng.standard_normal(H * K).astype(np.float32)
    w = np.concatenate([np.zeros(256, np.float32), a])[:256 * K]
    r = HC.live(a, w, x, 1.0, up, down, h)
    lat = rate_stream_latency(fs)
    assert r["lat"] == lat
    assert not r["s"].any() and not r["v"].any()
    want = np.concatenate([np.zeros(lat, np.float32), x])[:H * K]
    assert np.array_equal(r["out"], want.astype(np.float64))
    assert np.array_equal(r["bound"], 2 * 2.0 ** -24 * np.abs(want.astype(np.float64)))


def test_checker_states_the_contract_in_exact_arithmetic():
    """With w = R-invariant content the checker's output is R(w) + gamma (x delayed - lowpass(x) delayed): a tone above the
    band comes out with gain gamma, a tone inside it is left to the model path alone (48 kHz, float64 taps of the checker's
    own design, so this statement does not rest on the library)."""
    fs, K = 48000, 8
    upo, downo, _, ho = RC.design(16000, fs)
    upi, downi, halfi, hi = RC.design(fs, 16000)
    H, D = 768, 96
    n = np.arange(H * K)
    for f, carried in ((12000.0, True), (2000.0, False)):
        x = (0.25 * np.sin(2 * np.pi * f * n / fs)).astype(np.float32)
        a = RC.resample64(np.concatenate([np.zeros(D), x]), upi, downi, hi)[:256 * K].astype(np.float32)
        w = np.zeros(256 * K, np.float32)                                   # a model that removes everything
        r = HC.live(a, w, x, 0.5, upo, downo, ho.astype(np.float32))
        tail = r["out"][r["lat"] + 400:]
        amp = np.sqrt(2 * np.mean(tail ** 2))
        if carried:
            assert abs(amp - 0.125) < 1e-4, amp
        else:
            assert amp < 1e-4, amp
