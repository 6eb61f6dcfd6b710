"""CPU-side checks of the sample-rate conversion (gtcrn_resample_* / gtcrn_rate_stream_*): the coefficients against the
definition in float64, what the filter promises, the host-only size functions and argument checks, and -- in float64
numpy with a stand-in model -- the identity the live contract rests on (include/gtcrn_micro_hip.h)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import resample_checker as RC

RATE_SYMBOLS = ["gtcrn_resampler_create", "gtcrn_resampler_destroy", "gtcrn_resample_taps", "gtcrn_resample_out_len",
                "gtcrn_resample", "gtcrn_resample_pcm16_in", "gtcrn_resample_pcm16_out", "gtcrn_rate_stream_hop",
                "gtcrn_rate_stream_latency", "gtcrn_rate_stream_state_bytes", "gtcrn_rate_stream_reserve",
                "gtcrn_rate_stream_reset", "gtcrn_rate_stream_step", "gtcrn_rate_stream_step_pcm16"]
ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def test_rate_symbols_exported_and_abi_version_unchanged():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    for n in RATE_SYMBOLS:
        assert hasattr(L, n), n
    assert L.gtcrn_abi_version() == 1


@pytest.mark.parametrize("fs_in,fs_out", RC.PAIRS)
def test_taps_match_the_definition(fs_in, fs_out):
    """Each tap within 1 ulp (float32) of the float64 definition rounded to float32; sum(h) == up to 1e-6; symmetric."""
    from gtcrn_micro_amd._lib import resample_taps
    up, down, h = resample_taps(fs_in, fs_out)
    rup, rdown, half, h64 = RC.design(fs_in, fs_out)
    assert (up, down) == (rup, rdown)
    assert h.dtype == np.float32 and h.size == 2 * half + 1
    want = h64.astype(np.float32)
    ulp = np.spacing(np.abs(want))
    worst = float(np.max(np.abs(h.astype(np.float64) - want.astype(np.float64)) / ulp))
    print(f"{fs_in}->{fs_out}: up {up} down {down} taps {h.size} worst tap difference {worst:.2f} ulp")
    assert worst <= 1.0
    assert abs(float(h.astype(np.float64).sum()) - up) <= 1e-6 * up
    assert np.array_equal(h, h[::-1])


@pytest.mark.parametrize("fs_in,fs_out", RC.PAIRS)
def test_filter_keeps_its_promise(fs_in, fs_out):
    """From the returned float32 taps: within +-0.15 dB up to 0.875 of the lower Nyquist frequency, >= 90 dB down from
    1.125 x the lower Nyquist frequency to the Nyquist frequency of the tap grid."""
    from gtcrn_micro_amd._lib import resample_taps
    up, down, h = resample_taps(fs_in, fs_out)
    grid = fs_in * up
    nyq = min(fs_in, fs_out) / 2
    pb = RC.response_db(h, up, np.linspace(0, 0.875 * nyq, 200), grid)
    sb = RC.response_db(h, up, np.linspace(1.125 * nyq, grid / 2, 1500), grid)
    print(f"{fs_in}->{fs_out}: pass band {pb.min():+.4f} .. {pb.max():+.4f} dB, stop band {sb.max():.1f} dB")
    assert pb.max() <= 0.15 and pb.min() >= -0.15
    assert sb.max() <= -90.0


def test_identity_pair_is_one_tap():
    from gtcrn_micro_amd._lib import resample_taps, resample_out_len
    up, down, h = resample_taps(16000, 16000)
    assert (up, down) == (1, 1) and h.tolist() == [1.0]
    assert resample_out_len(16000, 16000, 777) == 777


def test_host_size_functions():
    from gtcrn_micro_amd import _lib
    for fs_in, fs_out in RC.PAIRS:
        up, down = RC.ratio(fs_in, fs_out)
        for L in (0, 1, 2, 255, 256, 257, 1000, 44100, 16000 * 600):
            assert _lib.resample_out_len(fs_in, fs_out, L) == RC.out_len(L, up, down), (fs_in, fs_out, L)
    # H = 256 fs / 16000; D = 32 q / up of fs -> 16000; latency H + 2 D: 20 ms, 24 ms at 8 kHz
    want = {8000: (128, 32), 24000: (384, 48), 32000: (512, 64), 48000: (768, 96)}
    for fs, (H, D) in want.items():
        up, down = RC.ratio(fs, 16000)
        assert D == 32 * max(up, down) // up
        assert _lib.rate_stream_hop(fs) == H
        assert _lib.rate_stream_latency(fs) == H + 2 * D
        assert _lib.rate_stream_latency(fs) * 1000 == (24 if fs == 8000 else 20) * fs
        # the two filters' histories as floats: the longest phase of each rounded up to a multiple of 4 taps
        nt_in = 64 * max(up, down) // up + 1
        nt_out = 64 * max(up, down) // down + 1
        assert _lib.rate_stream_state_bytes(fs) == 4 * ((nt_in + 3) // 4 * 4 + (nt_out + 3) // 4 * 4)
        assert _lib.rate_stream_state_bytes(fs) % 16 == 0


@pytest.mark.parametrize("fs", [0, -16000, 12345, 16001, 96000, 44101])
def test_unsupported_rates_are_rejected(fs):
    from gtcrn_micro_amd import _lib, GtcrnError
    L = _lib.lib()
    for a, b in ((fs, 16000), (16000, fs)):
        assert L.gtcrn_resample_taps(a, b, None, None, None, 0) == ERR_ARG
        assert L.gtcrn_resample_out_len(a, b, 100) == ERR_ARG
        h = ctypes.c_void_p()
        assert L.gtcrn_resampler_create(ctypes.byref(h), a, b, 0) == ERR_ARG and not h.value
    assert L.gtcrn_resample_taps(48000, 8000, None, None, None, 0) == ERR_ARG       # one side is always 16 kHz
    assert L.gtcrn_rate_stream_hop(fs) == ERR_ARG
    assert L.gtcrn_rate_stream_latency(fs) == ERR_ARG
    assert L.gtcrn_rate_stream_state_bytes(fs) == 0
    with pytest.raises(GtcrnError):
        _lib.resample_taps(fs, 16000)


@pytest.mark.parametrize("fs", [11025, 22050, 44100, 16000])
def test_offline_only_rates_have_no_live_form(fs):
    from gtcrn_micro_amd import _lib
    L = _lib.lib()
    assert L.gtcrn_rate_stream_hop(fs) == ERR_ARG
    assert L.gtcrn_rate_stream_state_bytes(fs) == 0


def test_null_pointers_are_argument_errors_before_the_device():
    from gtcrn_micro_amd._lib import lib
    L = lib()
    p = ctypes.c_void_p(16)           # never dereferenced: every call below is rejected before the device is touched
    calls = [
        lambda: L.gtcrn_resampler_create(None, 48000, 16000, 0),
        lambda: L.gtcrn_resample(None, p, 100, None, 100, p, 100, 1, None),
        lambda: L.gtcrn_resample_pcm16_in(None, p, 100, None, 100, p, 100, 1, None),
        lambda: L.gtcrn_resample_pcm16_out(None, p, 100, None, 100, p, 100, 1, None),
        lambda: L.gtcrn_rate_stream_reserve(None, p, p, 1, 1),
        lambda: L.gtcrn_rate_stream_reset(None, p, p, p, p, p, 1, None),
        lambda: L.gtcrn_rate_stream_step(None, p, p, p, p, p, p, 768, p, 768, 1, 1, p, None),
        lambda: L.gtcrn_rate_stream_step_pcm16(None, p, p, p, p, p, p, 768, p, 768, 1, 1, p, None),
    ]
    for i, c in enumerate(calls):
        assert c() == ERR_ARG, i
        assert b"null" in L.gtcrn_last_error(), i
    buf = (ctypes.c_float * 8)()
    assert L.gtcrn_resample_taps(48000, 16000, None, None, buf, 8) == ERR_ARG        # fewer than 2 half + 1 floats
    L.gtcrn_resampler_destroy(None)                                                  # a no-op


# ---------------------------------------------------------------- the live identity, restated in float64 numpy
def _stand_in_model(w, K):
    """A fixed block-causal map of 256-sample blocks (block k of the output depends on blocks <= k of the input), as the
    wave-to-wave model is away from the end-reflected last frame: a two-block FIR with a nonlinearity."""
    g = np.random.default_rng(5)
    A, Bm = g.standard_normal((256, 256)) / 16, g.standard_normal((256, 256)) / 16
    blocks = w[:256 * K].reshape(K, 256)
    prev = np.vstack([np.zeros((1, 256)), blocks[:-1]])
    return np.tanh(blocks @ A + prev @ Bm).reshape(-1)


def _causal_stage(x, hist, up, down, half, h, n_out):
    """The per-stream form: output m = sum_t h[k0 + t up] s[ih - t], ih = (m down) div up, k0 = (m down) mod up, over
    s = [history ++ this call's input]; returns (outputs, new history).  This is the centred filter delayed by half / down
    outputs."""
    nt = 2 * half // up + 1
    s = np.concatenate([hist, x])
    off = len(hist)
    y = np.zeros(n_out)
    for m in range(n_out):
        ih, k0 = divmod(m * down, up)
        t = np.arange((2 * half - k0) // up + 1)
        y[m] = np.sum(h[k0 + t * up] * s[off + ih - t])
    assert nt - 1 <= len(hist) <= len(s)
    return y, s[len(s) - len(hist):]


@pytest.mark.parametrize("fs", RC.LIVE_RATES)
def test_live_identity_in_float64(fs):
    """K hops through [causal fs -> 16k] -> [block-causal stand-in, one block late] -> [causal 16k -> fs], hop by hop
    with per-stream histories, against the centred offline chain on zeros(D) ++ x: out[n] == 0 for n < H and
    out[n] == u[n - H - D] for H + D <= n < H K, both with difference exactly 0 when both sides sum in one order
    (here: <= 1e-12, numpy's pairwise sums against scipy's convolution); and the 16 kHz hand-off equals the offline
    resampling delayed by 32 q / down samples."""
    K = 9
    up, down, half, h = RC.design(fs, 16000)
    upo, downo, halfo, ho = RC.design(16000, fs)
    H, D = 256 * down // up, half // up
    assert (H * up, D * up) == (256 * down, half) and halfo // downo == D
    rng = np.random.default_rng(fs)
    x = rng.standard_normal(H * K)
    # offline, centred
    y = RC.resample64(np.concatenate([np.zeros(D), x]), up, down, h)
    assert y.size == 256 * K + half // down
    w = _stand_in_model(y, K)                                     # forward_wave keeps 256 * floor(len / 256) samples
    u = RC.resample64(w, upo, downo, ho)
    # live, hop by hop
    nt_i, nt_o = 2 * half // up + 1, 2 * halfo // upo + 1
    hist_i, hist_o = np.zeros(nt_i + 3), np.zeros(nt_o + 3)
    prev_block, prev_in = np.zeros(256), np.zeros(256)
    A_state = []
    out, y_live = [], []
    g = np.random.default_rng(5)
    A, Bm = g.standard_normal((256, 256)) / 16, g.standard_normal((256, 256)) / 16
    for k in range(K):
        y16, hist_i = _causal_stage(x[k * H:(k + 1) * H], hist_i, up, down, half, h, 256)
        y_live.append(y16)
        blk = np.tanh(y16 @ A + prev_in @ Bm)                     # the stand-in's block k ...
        prev_in = y16
        v, prev_block = prev_block, blk                           # ... emitted one hop late, as the wave stream does
        o, hist_o = _causal_stage(v, hist_o, upo, downo, halfo, ho, H)
        out.append(o)
    out, y_live = np.concatenate(out), np.concatenate(y_live)
    dl = half // down
    yx = RC.resample64(x, up, down, h)
    np.testing.assert_allclose(y_live[dl:], yx[:256 * K - dl], rtol=0, atol=1e-12)      # stage: delayed by 32 q / down
    np.testing.assert_allclose(y_live, y[:256 * K], rtol=0, atol=1e-12)
    assert not out[:H].any()
    np.testing.assert_allclose(out[H + D:], u[:H * K - H - D], rtol=0, atol=1e-12)
