"""CPU-side checks of packet-sized live streaming (gtcrn_packet_stream_*, include/gtcrn_micro_hip.h): the host-only
geometry (n16, latency, state size, hop schedule) against the formulas of the contract, the argument checks that answer
before the device is touched, and -- in float64 numpy with real FIFOs, pre-roll joins, the causal stages and a block-causal
stand-in model -- the identity the live contract rests on."""
import ctypes
import os
from math import gcd

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import resample_checker as RC

PACKET_SYMBOLS = ["gtcrn_packet_stream_n16", "gtcrn_packet_stream_latency16", "gtcrn_packet_stream_state_bytes",
                  "gtcrn_packet_stream_schedule", "gtcrn_packet_stream_create", "gtcrn_packet_stream_destroy",
                  "gtcrn_packet_stream_phase", "gtcrn_packet_stream_next_hops", "gtcrn_packet_stream_reset",
                  "gtcrn_packet_stream_step", "gtcrn_packet_stream_step_pcm16", "gtcrn_packet_stream_debug_handoff"]
ERR_ARG = -1
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
N16_LIST = (1, 80, 96, 160, 256, 257, 320, 441, 640, 1000, 4096)


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _ntp(half, up):
    return (2 * half // up + 1 + 3) // 4 * 4


def geometry(fs, n):
    """The contract's formulas, from the rates alone: None for a packet the form does not take, else
    (n16, g, latency16, state floats, d_in, d_out)."""
    if fs not in RATES or n < 1 or (n * 16000) % fs:
        return None
    n16 = n * 16000 // fs
    if not 1 <= n16 <= 4096:
        return None
    g = gcd(n16, 256)
    if fs == 16000:
        return n16, g, 512 - g, 512, 0, 0
    up, down, half, _ = RC.design(fs, 16000)
    upo, downo, halfo, _ = RC.design(16000, fs)
    ntp_in, ntp_out = _ntp(half, up), _ntp(halfo, upo)
    if ntp_in > n or ntp_out > n16:
        return None
    assert half % down == 0 and halfo % upo == 0                 # whole stage delays at 16 kHz
    d_in, d_out = half // down, halfo // upo
    return n16, g, 512 - g + d_in + d_out, 512 + ntp_in + ntp_out, d_in, d_out


def packets_of(fs):
    ns = {1, 257}
    for ms in (10, 20, 40):
        if (fs * ms) % 1000 == 0:
            ns.add(fs * ms // 1000)
        else:
            ns.update((fs * ms // 1000, fs * ms // 1000 + 1))       # 220 / 221 at 22.05 kHz: not whole at 16 kHz
    if (256 * fs) % 16000 == 0:
        ns.add(256 * fs // 16000)
    if fs == 16000:
        ns.update((4096, 4097))
    return sorted(ns)


def test_packet_symbols_exported_and_abi_version_unchanged():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    for n in PACKET_SYMBOLS:
        assert hasattr(L, n), n
    assert L.gtcrn_abi_version() == 1


@pytest.mark.parametrize("fs", RATES)
def test_geometry_against_the_formulas(fs):
    """n16, latency16, the state size and the hop schedule over two periods for every packet of packets_of(fs); a packet
    the formulas reject is GTCRN_ERR_ARG / 0 bytes."""
    from gtcrn_micro_amd import _lib
    L = _lib.lib()
    accepted = 0
    for n in packets_of(fs):
        want = geometry(fs, n)
        if want is None:
            assert L.gtcrn_packet_stream_n16(fs, n) == ERR_ARG, (fs, n)
            assert L.gtcrn_packet_stream_latency16(fs, n) == ERR_ARG, (fs, n)
            assert L.gtcrn_packet_stream_state_bytes(fs, n) == 0, (fs, n)
            assert L.gtcrn_packet_stream_schedule(fs, n, 0, None) == ERR_ARG, (fs, n)
            continue
        accepted += 1
        n16, g, lat, floats, d_in, d_out = want
        assert _lib.packet_stream_n16(fs, n) == n16, (fs, n)
        assert _lib.packet_stream_latency16(fs, n) == lat, (fs, n)
        nbytes = _lib.packet_stream_state_bytes(fs, n)
        assert nbytes == 4 * floats and nbytes % 16 == 0, (fs, n)
        # never more than the two FIFOs of 256 + n16 and 512 + n16 floats and the histories
        assert nbytes <= 4 * ((256 + n16) + (512 + n16) + floats - 512), (fs, n)
        period, phi, hops = 256 // g, 0, 0
        for call in range(2 * period):
            h, nxt = _lib.packet_stream_schedule(fs, n, phi)
            assert h == (phi + n16) // 256 and nxt == (phi + n16) % 256, (fs, n, call)
            assert 0 <= 256 - g - phi < 256 and 256 - g - phi + 256 * h >= n16      # the outbound FIFO never underflows
            phi, hops = nxt, hops + h
            if call + 1 in (period, 2 * period):
                assert phi == 0 and hops * 256 == (call + 1) * n16, (fs, n, call)
            else:
                assert phi != 0, (fs, n, call)                                       # 256 / g is the SHORTEST period
        if g < 256:
            assert L.gtcrn_packet_stream_schedule(fs, n, g // 2 if g > 1 else 256, None) == ERR_ARG
    assert accepted >= 2, fs


def test_the_packets_of_the_contract():
    """10 ms passes at every accepted rate except 22.05 kHz, which takes 20 ms; the latencies the header names."""
    from gtcrn_micro_amd import _lib
    for fs in RATES:
        n = fs // 100
        if fs == 22050:
            assert geometry(fs, 220) is None and geometry(fs, 221) is None
            assert _lib.packet_stream_n16(fs, 441) == 320
        else:
            assert _lib.packet_stream_n16(fs, n) == 160
    assert [_lib.packet_stream_latency16(16000, n) for n in (256, 160, 320)] == [256, 480, 448]
    assert _lib.packet_stream_latency16(48000, 480) == 480 + 64
    assert _lib.packet_stream_latency16(8000, 80) == 480 + 128
    assert _lib.packet_stream_latency16(44100, 441) * 44100 / 16000 == pytest.approx(1499.4)
    assert _lib.packet_stream_latency16(48000, 768) * 3 == 960 == _lib.rate_stream_latency(48000)
    hs = []
    phi = 0
    for _ in range(8):
        h, phi = _lib.packet_stream_schedule(16000, 160, phi)
        hs.append(h)
    assert hs == [0, 1, 0, 1, 1, 0, 1, 1]                            # phases 0, 160, 64, 224, 128, 32, 192, 96


@pytest.mark.parametrize("fs,n", [(11025, 441), (11025, 110), (12345, 160), (0, 160), (-16000, 160), (96000, 960),
                                  (48000, 100), (44100, 440), (22050, 220), (24000, 241),              # not whole at 16 kHz
                                  (16000, 4097), (48000, 12291), (8000, 2049), (16000, 0), (16000, -160),
                                  (8000, 40), (48000, 96), (48000, 192), (44100, 147), (32000, 128)])  # shorter than a history
def test_unsupported_packets_are_rejected(fs, n):
    from gtcrn_micro_amd import _lib, GtcrnError
    L = _lib.lib()
    assert geometry(fs, n) is None
    assert L.gtcrn_packet_stream_n16(fs, n) == ERR_ARG
    assert L.gtcrn_packet_stream_latency16(fs, n) == ERR_ARG
    assert L.gtcrn_packet_stream_state_bytes(fs, n) == 0
    assert L.gtcrn_packet_stream_schedule(fs, n, 0, None) == ERR_ARG
    h = ctypes.c_void_p()
    p = ctypes.c_void_p(16)               # never dereferenced: the packet is rejected first
    assert L.gtcrn_packet_stream_create(ctypes.byref(h), p, None, None, fs, n, 4) == ERR_ARG and not h.value
    with pytest.raises(GtcrnError):
        _lib.packet_stream_n16(fs, n)
    with pytest.raises(GtcrnError):
        _lib.packet_stream_state_bytes(fs, n)


def test_null_pointers_are_argument_errors_before_the_device():
    from gtcrn_micro_amd._lib import lib
    L = lib()
    p = ctypes.c_void_p(16)               # never dereferenced: every call below is rejected before the device is touched
    h = ctypes.c_void_p()
    calls = [
        lambda: L.gtcrn_packet_stream_create(None, p, None, None, 16000, 160, 4),
        lambda: L.gtcrn_packet_stream_create(ctypes.byref(h), None, None, None, 16000, 160, 4),
        lambda: L.gtcrn_packet_stream_create(ctypes.byref(h), None, p, p, 48000, 480, 4),
        lambda: L.gtcrn_packet_stream_reset(None, p, p, p, 1, None),
        lambda: L.gtcrn_packet_stream_step(None, p, p, p, p, 160, p, 160, 1, p, None),
        lambda: L.gtcrn_packet_stream_step_pcm16(None, p, p, p, p, 160, p, 160, 1, p, None),
        lambda: L.gtcrn_packet_stream_phase(None),
        lambda: L.gtcrn_packet_stream_next_hops(None),
        lambda: L.gtcrn_packet_stream_debug_handoff(None, 0, p, 256, None),
    ]
    for i, c in enumerate(calls):
        assert c() == ERR_ARG, i
        assert b"null" in L.gtcrn_last_error(), i
    assert not h.value
    L.gtcrn_packet_stream_destroy(None)                                              # a no-op


# ---------------------------------------------------------------- the live identity, restated in float64 numpy
_G = np.random.default_rng(5)
_A, _B = _G.standard_normal((256, 256)) / 16, _G.standard_normal((256, 256)) / 16


def _stand_in_offline(w):
    """A fixed block-causal map of 256-sample blocks (block k of the output depends on blocks <= k of the input), as the
    wave-to-wave model is away from the end-reflected last frame; keeps 256 * floor(len / 256) samples."""
    K = len(w) // 256
    blocks = np.asarray(w[:256 * K], np.float64).reshape(K, 256)
    prev = np.vstack([np.zeros((1, 256)), blocks[:-1]])
    # block by block, the products the stepped form makes (a matrix-matrix product may sum in another order)
    return np.concatenate([np.tanh(blocks[k] @ _A + prev[k] @ _B) for k in range(K)] or [np.zeros(0)])


class _WaveStep:
    """The stand-in as gtcrn_wave_stream_step runs it: hop t in, block t - 1 out (zeros at t = 0)."""

    def __init__(self):
        self.prev_in, self.prev_block = np.zeros(256), np.zeros(256)

    def __call__(self, hop):
        blk = np.tanh(hop @ _A + self.prev_in @ _B)
        self.prev_in = hop
        out, self.prev_block = self.prev_block, blk
        return out


def _causal_stage(x, hist, up, down, half, h, n_out):
    """The per-stream causal stage on one packet: output m = sum_t h[k0 + t up] s[ih - t], ih = (m down) div up,
    k0 = (m down) mod up, over s = [history ++ the packet]; returns (outputs, new history)."""
    s = np.concatenate([hist, x])
    off = len(hist)
    y = np.zeros(n_out)
    for m in range(n_out):
        ih, k0 = divmod(m * down, up)
        t = np.arange((2 * half - k0) // up + 1)
        y[m] = np.sum(h[k0 + t * up] * s[off + ih - t])
    assert len(x) >= len(hist)                                   # the history comes out of ONE packet
    return y, s[len(s) - len(hist):]


class _Stream:
    """One stream of a group: real FIFOs pre-filled with the join's zeros, the two stage histories, the wave step."""

    def __init__(self, z, g, stages):
        self.z = z
        self.fin, self.fout = [0.0] * z, [0.0] * (256 - g - z)
        self.step = _WaveStep()
        self.stages = stages
        if stages:
            (up, down, half, h), (upo, downo, halfo, ho) = stages
            self.hist_i, self.hist_o = np.zeros(_ntp(half, up)), np.zeros(_ntp(halfo, upo))
        self.x, self.a16, self.b16, self.out = [], [], [], []

    def packet(self, x, n16, hops):
        self.x.append(x)
        if self.stages:
            up, down, half, h = self.stages[0]
            a, self.hist_i = _causal_stage(x, self.hist_i, up, down, half, h, n16)
        else:
            a = x
        self.a16.append(a)
        self.fin.extend(a)
        assert len(self.fin) // 256 == hops                      # every stream of the group steps the host's h
        for _ in range(hops):
            self.fout.extend(self.step(np.array(self.fin[:256])))
            del self.fin[:256]
        assert len(self.fout) >= n16, "outbound FIFO underflow"
        b = np.array(self.fout[:n16])
        del self.fout[:n16]
        self.b16.append(b)
        if self.stages:
            upo, downo, halfo, ho = self.stages[1]
            o, self.hist_o = _causal_stage(b, self.hist_o, upo, downo, halfo, ho, len(x))
        else:
            o = b
        self.out.append(o)


def _run_group(fs, n, ncalls, joins, seed):
    """A group at (fs, n) for ncalls calls; stream i joins before call joins[i] at the group's phase then."""
    n16, g = n * 16000 // fs, gcd(n * 16000 // fs, 256)
    stages = None if fs == 16000 else (RC.design(fs, 16000), RC.design(16000, fs))
    rng = np.random.default_rng(seed)
    streams, phi = {}, 0
    for call in range(ncalls):
        for i, j in enumerate(joins):
            if j == call:
                streams[i] = _Stream(phi, g, stages)
        hops = (phi + n16) // 256
        for s in streams.values():
            assert len(s.fin) == phi and len(s.fout) == 256 - g - phi      # the levels are the group's: nothing to store
            s.packet(rng.standard_normal(n), n16, hops)
        phi = (phi + n16) % 256
    return streams, n16, g


def _check_16k_identity(a16, b16, z, lat16, what):
    """b16 == zeros(L16 - z) ++ Y, Y = offline(zeros(z) ++ a16), over everything emitted: exactly (one order of sums)."""
    Y = _stand_in_offline(np.concatenate([np.zeros(z), a16]))
    lead = lat16 - z
    assert lead >= 0 and not b16[:lead].any(), what
    m = len(b16) - lead
    assert m <= len(Y), what                                     # nothing is emitted that the offline call has not got
    assert np.array_equal(b16[lead:], Y[:m]), what
    return m


@pytest.mark.parametrize("n16", N16_LIST)
def test_packet_identity_at_16k_in_float64(n16):
    """Joins after 0, 1, 3 and 7 calls, at least two periods and six hops: every stream obeys
    out == zeros(L16 - z) ++ forward(zeros(z) ++ x) with the z of its join, without an underflow."""
    period = 256 // gcd(n16, 256)
    ncalls = max(2 * period, -(-256 * 6 // n16)) + 8
    streams, _, g = _run_group(16000, n16, ncalls, (0, 1, 3, 7), n16)
    zs = set()
    for i, s in streams.items():
        x, out = np.concatenate(s.x), np.concatenate(s.out)
        assert out.shape == x.shape
        got = _check_16k_identity(x, out, s.z, 512 - g, (n16, i))
        assert got > 0 or n16 < 4, (n16, i)
        zs.add(s.z)
    assert streams[0].z == 0 and (len(zs) > 1 or g == 256)


@pytest.mark.parametrize("fs,n", [(8000, 80), (44100, 441), (48000, 480), (22050, 441)])
def test_packet_identity_at_other_rates_in_float64(fs, n):
    """Stage by stage: the 16 kHz hand-off is the centred resampling delayed by d_in (pre-ringing in front), the 16 kHz
    identity holds on it exactly, and the output is the centred resampling of zeros(d_out) ++ b16.  Against scipy's
    convolution: <= 1e-12."""
    n16, g, lat, _, d_in, d_out = geometry(fs, n)
    period = 256 // g
    ncalls = 2 * period + 3
    streams, _, _ = _run_group(fs, n, ncalls, (0, 1, 3), fs + n)
    up, down, half, h = RC.design(fs, 16000)
    upo, downo, halfo, ho = RC.design(16000, fs)
    for i, s in streams.items():
        x, a16, b16, out = (np.concatenate(v) for v in (s.x, s.a16, s.b16, s.out))
        assert out.shape == x.shape and a16.size == b16.size == n16 * len(s.x)
        c = -(-d_in // up)
        ref = RC.resample64(np.concatenate([np.zeros(c * down), x]), up, down, h)[c * up - d_in:][:a16.size]
        np.testing.assert_allclose(a16, ref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(a16[d_in:], RC.resample64(x, up, down, h)[:a16.size - d_in], rtol=0, atol=1e-12)
        assert _check_16k_identity(a16, b16, s.z, lat - d_in - d_out, (fs, n, i)) > 0
        u = RC.resample64(np.concatenate([np.zeros(d_out), b16]), upo, downo, ho)[:out.size]
        np.testing.assert_allclose(out, u, rtol=0, atol=1e-12)
    assert any(s.z for s in streams.values())
