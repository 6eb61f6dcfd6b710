"""Hop-level waveform streaming (gtcrn_wave_stream_*): 256 samples in, 256 enhanced out per stream and call, equal to
gtcrn_forward_wave one hop late, bit for bit (contract: include/gtcrn_micro_hip.h)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_params

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as graft
    graft.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(dev):
    from gtcrn_micro_amd import Engine
    return Engine(load_params("dns3"), 0)


@pytest.fixture(scope="module")
def win(dev):
    return torch.hann_window(512).pow(0.5).cuda()                   # exactly what infer.py:65 passes


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream_clip(eng, st, x, chunks=None):
    """x (N, L) -> the streamed output (N, 256 (L // 256 + 1)): whole hops in calls of `chunks` hops (cycled), then
    the flush with the rest."""
    K = x.shape[1] // 256
    chunks = chunks or [1]
    outs, k, i = [], 0, 0
    while k < K:
        nh = min(chunks[i % len(chunks)], K - k)
        outs.append(eng.wave_stream_step(st, x[:, 256 * k:256 * (k + nh)]))
        k += nh
        i += 1
    outs.append(eng.wave_stream_flush(st, x[:, 256 * K:]))
    return torch.cat(outs, 1)


@pytest.fixture(scope="module")
def examples():
    return np.load(os.path.join(GOLDEN, "examples_full.npz"))


def test_wave_equals_stft_model_istft_bit_for_bit(eng, win, examples):
    """What the streamed identity rests on: the fused offline path (k_front's STFT) equals stft -> forward_spec -> istft
    bit for bit -- checked first, so that a difference is located before the wave-stream kernels are blamed."""
    import gtcrn_micro_amd as G
    x = cu(examples["noisy"][:, :256 * 200 + 77].astype(np.float32) / 32768.0)
    y = eng.forward_wave(x, win)
    assert torch.equal(G.istft(eng.forward_spec(G.stft(x, win)), win), y)


def test_five_reference_clips_streamed_hop_by_hop(eng, win, examples):
    """The five reference clips (1 937 hops + 128 samples), five streams side by side, one hop per call, then the
    flush: out[:, 256:] == forward_wave bit for bit, out[:, :256] == 0, and so within 1.05 LSB of enh{1..5}.wav.
    Then clip 1 alone in ragged calls of 1, 2, 5, 16, 33, ... hops: the same bits."""
    x = cu(examples["noisy"].astype(np.float32) / 32768.0)
    assert x.shape == (5, 496000)
    ref = eng.forward_wave(x, win)
    st = eng.new_wave_state(5, win)
    out = stream_clip(eng, st, x)
    assert out.shape == (5, 496128)
    assert not out[:, :256].any()
    assert torch.equal(out[:, 256:], ref)
    lsb = np.abs(out[:, 256:].cpu().numpy().astype(np.float64) * 32768.0 - examples["enh"]).max(axis=1)
    print("wave-streamed, max deviation from enhN.wav in LSB:", np.round(lsb, 4))
    assert (lsb <= 1.05).all(), lsb
    st1 = eng.new_wave_state(1, win)
    out1 = stream_clip(eng, st1, x[:1], chunks=[1, 2, 5, 16, 33, 3, 64, 7])
    assert torch.equal(out1, out[:1])


LENGTHS = [(K, r) for K in (1, 2, 3, 40) for r in (0, 1, 100, 255) if (K, r) != (1, 0)]   # L = 256 < 257: no clip


@pytest.mark.parametrize("K,r", LENGTHS)
def test_any_length(eng, win, K, r):
    """L = 256 K + r: steps + flush give forward_wave's samples after the 256 zeros.  K = 1: frame 0 and the end
    reflection overlap and the ring holds hop 0 only."""
    gen = torch.Generator(device="cuda").manual_seed(1000 * K + r)
    x = torch.randn(3, 256 * K + r, device="cuda", generator=gen) * 0.1
    st = eng.new_wave_state(3, win)
    out = stream_clip(eng, st, x, chunks=[1, 2])
    assert out.shape == (3, 256 * (K + 1))
    assert not out[:, :256].any()
    assert torch.equal(out[:, 256:], eng.forward_wave(x, win))


@pytest.mark.parametrize("N", [1024, 8192])
def test_many_streams_at_different_phases(eng, win, N):
    """Seeded random streams, ragged hops per call, a sub-range reset mid-run: every stream's output since its reset is
    forward_wave of the samples pushed since then, one hop late (all but the last block, which belongs to the flush).
    The same bits in every form of the model step (default, three launches, four / seven streams per workgroup)."""
    from gtcrn_micro_amd._lib import stream_streams_per_workgroup
    assert stream_streams_per_workgroup(N) == (4 if N == 1024 else 7)
    gen = torch.Generator(device="cuda").manual_seed(N)
    H = 14
    x = torch.randn(N, 256 * H, device="cuda", generator=gen) * 0.1
    lo, hi, R = N // 5, N // 5 + N // 3, 5                          # streams lo..hi-1 restart after hop R
    sched = [1, 2, 1, 1, 3, 2, 1, 3]
    assert sum(sched) == H and sum(sched[:4]) == R
    results = []
    for form in (0, 1, 2, 3):
        eng.stream_form(form)
        try:
            st = eng.new_wave_state(N, win)
            outs, k = [], 0
            for nh in sched:
                if k == R:
                    eng.wave_stream_reset(st, lo, hi)
                outs.append(eng.wave_stream_step(st, x[:, 256 * k:256 * (k + nh)]))
                k += nh
            results.append(torch.cat(outs, 1))
        finally:
            eng.stream_form(0)
    out = results[0]
    keep = torch.ones(N, dtype=torch.bool, device="cuda")
    keep[lo:hi] = False
    ref = eng.forward_wave(x[keep], win)
    assert not out[keep, :256].any()
    assert torch.equal(out[keep, 256:256 * H], ref[:, :256 * (H - 1)])
    ref_r = eng.forward_wave(x[lo:hi, 256 * R:], win)
    assert not out[lo:hi, 256 * R:256 * (R + 1)].any()
    assert torch.equal(out[lo:hi, 256 * (R + 1):], ref_r[:, :256 * (H - R - 1)])
    for form, o in zip((1, 2, 3), results[1:]):
        assert torch.equal(o, out), form


def test_pcm16_equals_float_between_the_converters(eng, win, examples):
    """The int16 step == f32_to_pcm16(float step of pcm16_to_f32(x)), bit for bit, steps and flush."""
    from gtcrn_micro_amd import f32_to_pcm16, pcm16_to_f32
    x16 = cu(examples["noisy"][:, :256 * 60 + 40])
    xf = pcm16_to_f32(x16[:, :256 * 60].contiguous())
    tf = x16[:, 256 * 60:].float() / 32768.0
    sa, sb = eng.new_wave_state(5, win), eng.new_wave_state(5, win)
    for k in range(0, 60, 3):
        y16 = eng.wave_stream_step(sa, x16[:, 256 * k:256 * (k + 3)])
        yf = eng.wave_stream_step(sb, xf[:, 256 * k:256 * (k + 3)])
        assert y16.dtype == torch.int16
        assert torch.equal(y16, f32_to_pcm16(yf.contiguous())), k
    y16 = eng.wave_stream_flush(sa, x16[:, 256 * 60:])
    yf = eng.wave_stream_flush(sb, tf)
    assert torch.equal(y16, f32_to_pcm16(yf.contiguous()))


def test_wave_step_is_graph_capturable(eng, win):
    """After reserve(N, 1) one wave step captures into a HIP graph (one stream, no parallel branches); replayed over 64
    hops with new samples copied into the captured buffer it gives the eager run's outputs and states."""
    N, H = 16, 64
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, 256 * H, device="cuda", generator=gen) * 0.1
    eng.reserve(N, 1)
    ref_st = eng.new_wave_state(N, win)
    ref = [eng.wave_stream_step(ref_st, x[:, 256 * t:256 * (t + 1)]).clone() for t in range(H)]
    xb = torch.empty(N, 256, device="cuda")
    yb = torch.empty(N, 256, device="cuda")
    st = eng.new_wave_state(N, win)
    warm = eng.new_wave_state(N, win)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        xb.copy_(x[:, :256])
        eng.wave_stream_step(warm, xb, out=yb)                       # warm-up on the capture stream (another state)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            eng.wave_stream_step(st, xb, out=yb)
    eng.wave_stream_reset(st)                                        # the capture itself did not run the step
    torch.cuda.synchronize()
    for t in range(H):
        xb.copy_(x[:, 256 * t:256 * (t + 1)])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yb, ref[t]), t
    assert torch.equal(st.model, ref_st.model)
    assert torch.equal(st.wave, ref_st.wave)


def test_bad_arguments_raise_and_leave_the_output_alone(eng, win):
    import ctypes
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import lib
    N = 4
    st = eng.new_wave_state(N, win)
    x = torch.zeros(N, 512, device="cuda")
    out = torch.full((N, 512), 7.0, device="cuda")
    bad_win = win.clone()
    bad_win[0] = 1e-3
    with pytest.raises(GtcrnError):
        eng.new_wave_state(N, bad_win)                               # window[0] != 0
    with pytest.raises(GtcrnError):
        eng.new_wave_state(N, win[:256])
    for bad in (torch.zeros(N, 300, device="cuda"), torch.zeros(N + 1, 512, device="cuda"),
                torch.zeros(N, 512, device="cuda", dtype=torch.float64), torch.zeros(N, 0, device="cuda")):
        with pytest.raises(GtcrnError):
            eng.wave_stream_step(st, bad, out=out)
    with pytest.raises(GtcrnError):
        eng.wave_stream_step(st, x, out=torch.empty(N, 256, device="cuda"))
    with pytest.raises(GtcrnError):
        eng.wave_stream_flush(st, torch.zeros(N, 256, device="cuda"), out=out[:, :256])
    with pytest.raises(GtcrnError):
        eng.wave_stream_reset(st, 3, 2)
    L, h, sp = lib(), eng._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    m, w, xi, o, wi = st.model.data_ptr(), st.wave.data_ptr(), x.data_ptr(), out.data_ptr(), st.window.data_ptr()
    calls = [
        lambda: L.gtcrn_wave_stream_step(None, m, w, xi, 512, o, 512, N, 2, wi, sp),
        lambda: L.gtcrn_wave_stream_step(h, None, w, xi, 512, o, 512, N, 2, wi, sp),
        lambda: L.gtcrn_wave_stream_step(h, m, None, xi, 512, o, 512, N, 2, wi, sp),
        lambda: L.gtcrn_wave_stream_step(h, m, w, None, 512, o, 512, N, 2, wi, sp),
        lambda: L.gtcrn_wave_stream_step(h, m, w, xi, 512, None, 512, N, 2, wi, sp),
        lambda: L.gtcrn_wave_stream_step(h, m, w, xi, 512, o, 512, N, 2, None, sp),
        lambda: L.gtcrn_wave_stream_step(h, m, w, xi, 512, o, 512, 0, 2, wi, sp),
        lambda: L.gtcrn_wave_stream_step(h, m, w, xi, 512, o, 512, N, 0, wi, sp),
        lambda: L.gtcrn_wave_stream_step(h, m, w, xi, 511, o, 512, N, 2, wi, sp),
        lambda: L.gtcrn_wave_stream_step(h, m, w, xi, 512, o, 300, N, 2, wi, sp),
        lambda: L.gtcrn_wave_stream_flush(h, m, w, xi, 512, 256, o, 512, N, wi, sp),
        lambda: L.gtcrn_wave_stream_flush(h, m, w, xi, 512, -1, o, 512, N, wi, sp),
        lambda: L.gtcrn_wave_stream_flush(h, m, w, None, 512, 5, o, 512, N, wi, sp),
        lambda: L.gtcrn_wave_stream_flush(h, m, w, xi, 4, 5, o, 512, N, wi, sp),
        lambda: L.gtcrn_wave_stream_flush(h, m, w, xi, 512, 5, o, 255, N, wi, sp),
        lambda: L.gtcrn_wave_stream_step_pcm16(h, m, w, xi, 512, o, 512, N, 0, wi, sp),
        lambda: L.gtcrn_wave_stream_flush_pcm16(h, m, w, xi, 512, 300, o, 512, N, wi, sp),
        lambda: L.gtcrn_wave_stream_reset(h, None, w, N, sp),
        lambda: L.gtcrn_wave_stream_reset(h, m, w, 0, sp),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i                                          # GTCRN_ERR_ARG
        assert L.gtcrn_last_error(), i
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert not st.wave.any()                                         # nothing ran: the wave state is still reset
