"""CPU-side checks of hop-level waveform streaming (gtcrn_wave_stream_*): the ABI, the window precondition and, in
float64, the identity the one-hop-delay contract rests on (include/gtcrn_micro_hip.h)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft

torch = pytest.importorskip("torch")

WAVE_SYMBOLS = ["gtcrn_wave_stream_state_bytes", "gtcrn_wave_stream_reset", "gtcrn_wave_stream_step",
                "gtcrn_wave_stream_step_pcm16", "gtcrn_wave_stream_flush", "gtcrn_wave_stream_flush_pcm16"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def test_wave_symbols_exported_and_state_size():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    for n in WAVE_SYMBOLS:
        assert hasattr(L, n), n
    from gtcrn_micro_amd import Engine
    # input ring 512 + overlap-add tail 256 + hop counter (+ pad), floats; rows 16-byte aligned
    assert Engine.wave_state_bytes() == 4 * (512 + 256 + 4) == 3088
    assert Engine.wave_state_bytes() % 16 == 0


def test_windows_start_at_exact_zero():
    """Frame 0 of torch.stft(center=True) reads one future sample, x[256], at win[0]: the contract needs win[0] == 0."""
    from gtcrn_micro_amd import make_window
    assert torch.hann_window(512).pow(0.5)[0].item() == 0.0
    assert make_window(0)[0] == 0.0
    assert make_window(1)[0] == 0.0


def test_null_model_and_null_pointers_are_argument_errors():
    from gtcrn_micro_amd._lib import lib
    L = lib()
    p = ctypes.c_void_p(16)           # never dereferenced: every call below is rejected before the device is touched
    ERR_ARG = -1
    calls = [
        lambda: L.gtcrn_wave_stream_reset(None, p, p, 1, None),
        lambda: L.gtcrn_wave_stream_step(None, p, p, p, 256, p, 256, 1, 1, p, None),
        lambda: L.gtcrn_wave_stream_step_pcm16(None, p, p, p, 256, p, 256, 1, 1, p, None),
        lambda: L.gtcrn_wave_stream_flush(None, p, p, p, 256, 10, p, 256, 1, p, None),
        lambda: L.gtcrn_wave_stream_flush_pcm16(None, p, p, p, 256, 10, p, 256, 1, p, None),
    ]
    for i, c in enumerate(calls):
        assert c() == ERR_ARG, i
        assert b"null model" in L.gtcrn_last_error(), i


# ---------------------------------------------------------------- the identity, restated in float64 with torch
def _stream_in_hops(x, w):
    """Per-hop framing + overlap-add with one hop of delay, as the kernels do it: call k frames hop k (hop k-1 from
    the ring; frame 0 start-reflected with its future sample read as 0), emits block k-1 = tail + first half of frame
    k over the envelope; the flush frames the end-reflected rest.  Returns the output stream, 256 (K + 1) samples."""
    L = x.numel()
    K, r = divmod(L, 256)
    env = w[256:] ** 2 + w[:256] ** 2

    def through(frame):              # the model is the identity here: rfft -> irfft, windowed twice
        return torch.fft.irfft(torch.fft.rfft(frame * w), n=512) * w

    out, tail = [], torch.zeros(256, dtype=torch.float64)
    ring = torch.zeros(512, dtype=torch.float64)
    for k in range(K):
        hop = x[256 * k:256 * (k + 1)]
        if k == 0:
            frame = torch.cat([torch.zeros(1, dtype=torch.float64), hop.flip(0)[:255], hop])
        else:
            frame = torch.cat([ring[256:], hop])
        f = through(frame)
        out.append(torch.zeros(256, dtype=torch.float64) if k == 0 else (tail + f[:256]) / env)
        tail = f[256:]
        ring = torch.cat([ring[256:], hop])
    buf = torch.cat([ring, x[256 * K:]])                            # [last 512 ++ the r extra samples]
    idx = torch.arange(256, 768)
    rl = 512 + r
    idx = torch.where(idx >= rl, 2 * (rl - 1) - idx, idx)
    f = through(buf[idx])
    out.append((tail + f[:256]) / env)
    return torch.cat(out)


LENGTHS = [(K, r) for K in (1, 2, 3, 40) for r in (0, 1, 100, 255) if (K, r) != (1, 0)]   # L = 256: no offline clip


@pytest.mark.parametrize("K,r", LENGTHS)
def test_hop_framing_with_one_hop_delay_is_stft_istft(K, r):
    """For L = 256 K + r >= 257: the per-hop stream equals torch.istft(torch.stft(x, center=True)) delayed by one hop
    (float64, the model replaced by the identity; the future sample of frame 0 read as 0, where it meets win[0] == 0)."""
    L = 256 * K + r
    g = torch.Generator().manual_seed(L)
    x = torch.randn(L, generator=g, dtype=torch.float64)
    w = torch.hann_window(512, dtype=torch.float64).pow(0.5)
    assert w[0].item() == 0.0
    spec = torch.stft(x, 512, 256, 512, w, center=True, pad_mode="reflect", return_complex=True)
    assert spec.shape[1] == K + 1
    off = torch.istft(spec, 512, 256, 512, w, center=True, length=256 * K)
    got = _stream_in_hops(x, w)
    assert got.numel() == 256 * (K + 1)
    assert not got[:256].any()
    np.testing.assert_allclose(got[256:].numpy(), off.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(off.numpy(), x[:256 * K].numpy(), rtol=0, atol=1e-12)   # (perfect reconstruction)
