"""CPU-side checks of the high band on the packet forms (gtcrn_packet_stream_step_hb / _step_slots_hb,
include/gtcrn_micro_hip.h "high band on the packet forms"): the symbols and their declarations, the latency and the size of
the new state for the packets the header lists, the (fs, n) without a high band, the sizes the feature must leave alone, the
argument errors that are returned without a device, and the checker of the contract (tests/highband_packet_checker.py) on
the case the contract makes exact and on two tones in float64."""
import ctypes
import os
from math import gcd

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import highband_packet_checker as PC
import resample_checker as RC

SYMBOLS = ["gtcrn_packet_stream_hb_latency", "gtcrn_packet_stream_hb_state_bytes", "gtcrn_packet_stream_hb_reset",
           "gtcrn_packet_stream_hb_reset_slots", "gtcrn_packet_stream_step_hb", "gtcrn_packet_stream_step_hb_pcm16",
           "gtcrn_packet_stream_step_slots_hb", "gtcrn_packet_stream_step_slots_hb_pcm16"]
# (fs, n): LAT in samples at fs, as the header lists them
TABLE = {(48000, 480): 1632, (48000, 960): 1536, (48000, 768): 960, (32000, 320): 1088, (24000, 240): 816, (24000, 480): 768}
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
    for n in SYMBOLS:
        assert hasattr(raw, n), n
        assert n + "(" in header, n
    assert raw.gtcrn_abi_version() == 1


def test_latency_and_state_size(L):
    """LAT = latency16 * fs / 16000 and a row of L16 + LAT floats rounded up to a multiple of 4 floats."""
    from gtcrn_micro_amd import _lib
    for (fs, n), lat in TABLE.items():
        n16 = n * 16000 // fs
        l16 = 512 - gcd(n16, 256)
        assert _lib.packet_stream_latency16(fs, n) == l16 + 64
        assert L.gtcrn_packet_stream_hb_latency(fs, n) == lat == (l16 + 64) * fs // 16000, (fs, n)
        assert _lib.packet_stream_hb_latency(fs, n) == lat
        want = 4 * ((l16 + lat + 3) // 4 * 4)
        assert L.gtcrn_packet_stream_hb_state_bytes(fs, n) == want, (fs, n)
        assert _lib.packet_stream_hb_state_bytes(fs, n) == want and want % 16 == 0
    assert L.gtcrn_packet_stream_hb_state_bytes(48000, 480) == 8448


def test_no_high_band_elsewhere(L):
    """8 / 16 kHz have no band above 8 kHz, the 44.1 kHz family no whole latency.  At 24 kHz the latency is whole for an even
    n16 only -- and a whole packet of n samples at 24 kHz HAS an even n16 = 2 n / 3, so the odd case reaches the library only
    as a packet that is no whole number of 16 kHz samples, which the packet form itself refuses."""
    from gtcrn_micro_amd import _lib
    bad = [(8000, 80), (8000, 160), (16000, 160), (16000, 320), (22050, 441), (44100, 441), (44100, 882), (24000, 241),
           (24000, 242), (48000, 481), (48000, 0), (0, 480), (11025, 441)]
    for fs, n in bad:
        assert L.gtcrn_packet_stream_hb_latency(fs, n) == ERR_ARG, (fs, n)
        assert b"high band" in L.gtcrn_last_error(), (fs, n)
        assert L.gtcrn_packet_stream_hb_state_bytes(fs, n) == 0, (fs, n)
        assert b"high band" in L.gtcrn_last_error(), (fs, n)
        with pytest.raises(_lib.GtcrnError):
            _lib.packet_stream_hb_latency(fs, n)
        with pytest.raises(_lib.GtcrnError):
            _lib.packet_stream_hb_state_bytes(fs, n)
    for n in range(3, 1200, 3):                                     # every whole packet at 24 kHz: n16 is even
        assert (n * 16000 // 24000) % 2 == 0


def test_packet_state_bytes_are_what_they_were(L):
    """Two FIFOs of 256 floats and the two filter histories: the formula of the packet form, unchanged."""
    for (fs, n) in TABLE:
        up, down = RC.ratio(fs, 16000)
        nt_in, nt_out = 64 * max(up, down) // up + 1, 64 * max(up, down) // down + 1
        assert L.gtcrn_packet_stream_state_bytes(fs, n) == 4 * (512 + (nt_in + 3) // 4 * 4 + (nt_out + 3) // 4 * 4), (fs, n)
    assert L.gtcrn_packet_stream_state_bytes(16000, 160) == 4 * 512
    assert L.gtcrn_packet_stream_latency16(48000, 480) == 544


def test_argument_errors_are_returned_without_a_device(L):
    p = ctypes.c_void_p(16)           # never dereferenced: every call below is rejected before the device is touched
    calls = [
        lambda: L.gtcrn_packet_stream_step_hb(None, p, p, p, p, 480, p, 480, 1, p, p, p, None),
        lambda: L.gtcrn_packet_stream_step_hb_pcm16(None, p, p, p, p, 480, p, 480, 1, p, p, p, None),
        lambda: L.gtcrn_packet_stream_step_slots_hb(None, p, p, p, p, p, None, 1, p, 480, p, 480, p, p, p, None),
        lambda: L.gtcrn_packet_stream_step_slots_hb_pcm16(None, p, p, p, p, p, None, 1, p, 480, p, 480, p, p, p, None),
        lambda: L.gtcrn_packet_stream_hb_reset(None, p, 1, None),
        lambda: L.gtcrn_packet_stream_hb_reset_slots(None, p, p, None, 1, None),
    ]
    for i, c in enumerate(calls):
        assert c() == ERR_ARG, i
        assert L.gtcrn_last_error(), i


def _taps32(fs):
    from gtcrn_micro_amd._lib import resample_taps
    return resample_taps(16000, fs)


@pytest.mark.parametrize("fs,n", sorted(TABLE))
def test_checker_bypass_is_exact(fs, n):
    """P = A delayed by L16 (what the attenuation limit at 0 dB guarantees) and gamma = 1: s == 0, v == 0 and the checker
    returns x delayed by LAT exactly, with a bound of two roundings of x alone."""
    up, down, h = _taps32(fs)
    n16, K = n * 16000 // fs, 9
    l16 = 512 - gcd(n16, 256)
    rng = np.random.default_rng(fs + n)
    A = rng.standard_normal(n16 * K).astype(np.float32)
    x = rng.standard_normal(n * K).astype(np.float32)
    P = np.concatenate([np.zeros(l16, np.float32), A])[:n16 * K]
    r = PC.live(A, P, x, 1.0, l16, 32, up, down, h)
    assert r["lat"] == TABLE[(fs, n)]
    assert not r["s"].any() and not r["v"].any()
    want = np.concatenate([np.zeros(r["lat"], np.float32), x])[:n * K]
    assert want[r["lat"]:].any()
    assert np.array_equal(r["out"], want.astype(np.float64))
    assert np.array_equal(r["bound"], 2 * 2.0 ** -24 * np.abs(want.astype(np.float64)))


@pytest.mark.parametrize("fs,n,f", [(48000, 480, 12000.0), (24000, 240, 10000.0)])
def test_checker_states_the_contract_in_exact_arithmetic(fs, n, f):
    """With a model that removes everything (P == 0) and gamma = 0.5 the checker's output is gamma (x delayed by LAT minus
    its low band, delayed alike): a tone above the band comes out at gamma times its amplitude, a 2 kHz tone cancels
    (float64 taps of the checker's own design, so this statement does not rest on the library).  Measured: 1e-9 and 6e-7."""
    upo, downo, _, ho = RC.design(16000, fs)
    upi, downi, halfi, hi = RC.design(fs, 16000)
    d16 = halfi // downi
    assert d16 == 32 and (d16 * downi) % upi == 0
    D = d16 * downi // upi                                          # the inbound stage's delay in samples at fs
    n16, K = n * 16000 // fs, 24
    l16 = 512 - gcd(n16, 256)
    t = np.arange(n * K)
    for tone, carried in ((f, True), (2000.0, False)):
        x = (0.25 * np.sin(2 * np.pi * tone * t / fs)).astype(np.float32)
        A = RC.resample64(np.concatenate([np.zeros(D), x]), upi, downi, hi)[:n16 * K].astype(np.float32)
        P = np.zeros(n16 * K, np.float32)
        r = PC.live(A, P, x, 0.5, l16, 32, upo, downo, ho.astype(np.float32))
        assert r["lat"] == TABLE[(fs, n)]
        tail = r["out"][r["lat"] + 400:]
        amp = np.sqrt(2 * np.mean(tail ** 2))
        print(f"fs {fs} n {n} tone {tone}: amplitude {amp:.3e}")
        if carried:
            assert abs(amp - 0.125) < 1e-4, amp
        else:
            assert amp < 1e-4, amp
