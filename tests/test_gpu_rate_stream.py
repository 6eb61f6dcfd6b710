"""Hop-level streaming at the caller's rate (gtcrn_rate_stream_*): H = 256 fs / 16000 samples in, H enhanced out per stream
and call, equal to resample -> gtcrn_forward_wave -> resample on the delayed signal, bit for bit (contract:
include/gtcrn_micro_hip.h)."""
import ctypes

import numpy as np
import pytest

from conftest import load_params
import resample_checker as RC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GEOM = {8000: (128, 32), 24000: (384, 48), 32000: (512, 64), 48000: (768, 96)}      # fs: (H, D)


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
    return torch.hann_window(512).pow(0.5).cuda()


def run_stream(eng, st, x, chunks, resets=None, taps=None):
    """x (N, H K) in calls of `chunks` hops (cycled); resets = {hop index: (lo, hi)}: those streams are reset before the
    call that starts at that hop (the schedule puts a call boundary there).  taps: list that receives each call's 16 kHz
    hand-off."""
    H, K = st.hop, x.shape[1] // st.hop
    resets = resets or {}
    outs, k, i = [], 0, 0
    while k < K:
        if k in resets:
            eng.rate_stream_reset(st, *resets[k])
        nh = min(chunks[i % len(chunks)], K - k)
        nxt = min([r for r in resets if r > k] + [K])
        nh = min(nh, nxt - k)
        outs.append(eng.rate_stream_step(st, x[:, H * k:H * (k + nh)]))
        if taps is not None:
            taps.append(eng.rate_stream_handoff(st, nh, 0))
        k += nh
        i += 1
    return torch.cat(outs, 1)


def check_identity(eng, win, fs, out, x, what):
    """One stream's output `out` for its input x (both 1-D, H K samples; float32): zeros for n < H, then
    u[n - H - D] from H + D on, u = forward_wave_rate(zeros(D) ++ x, fs, win, out_fs=fs)."""
    H, D = GEOM[fs]
    K = x.numel() // H
    u = eng.forward_wave_rate(torch.cat([torch.zeros(D, device="cuda"), x]), fs, win, out_fs=fs)
    o, uu = out.cpu().numpy(), u.cpu().numpy()
    assert not o[:H].any(), what
    assert uu.size >= H * K - H - D
    assert np.array_equal(o[H + D:], uu[:H * K - H - D]), (what, int((o[H + D:] != uu[:H * K - H - D]).sum()))


@pytest.mark.parametrize("fs", RC.LIVE_RATES)
@pytest.mark.parametrize("N", [1, 6])
def test_live_identity_bit_for_bit(eng, win, fs, N):
    """K = 23 hops in calls of 1, 2 and 5 hops mixed; with N = 6, streams 1..2 are reset before hop 8 and stream 4 before
    hop 13: every (stream, segment since its reset) obeys the identity on its own.  Stage by stage as well: the 16 kHz
    samples k_rate_in hands over equal gtcrn_resample(x) delayed by 32 q / down samples (the first of them: the
    resampling of zeros(D) ++ x)."""
    from gtcrn_micro_amd._lib import rate_stream_hop, rate_stream_latency
    H, D = GEOM[fs]
    assert rate_stream_hop(fs) == H and rate_stream_latency(fs) == H + 2 * D
    K = 23
    gen = torch.Generator(device="cuda").manual_seed(fs + N)
    x = torch.randn(N, H * K, device="cuda", generator=gen) * 0.1
    st = eng.new_rate_state(N, win, fs)
    assert st.hop == H and st.latency == H + 2 * D and st.fs == fs
    resets = {8: (1, 3), 13: (4, 5)} if N > 1 else {}
    taps = []
    out = run_stream(eng, st, x, [1, 2, 5], resets, taps)
    assert out.shape == x.shape
    starts = {n: 0 for n in range(N)}
    ends = {n: [] for n in range(N)}
    for k, (lo, hi) in sorted(resets.items()):
        for n in range(lo, hi):
            ends[n].append((starts[n], k))
            starts[n] = k
    for n in range(N):
        for a, b in ends[n] + [(starts[n], K)]:
            check_identity(eng, win, fs, out[n, H * a:H * b], x[n, H * a:H * b], f"fs {fs} stream {n} hops {a}..{b}")
    # the hand-off of k_rate_in (streams that were never reset)
    y16 = torch.cat(taps, 1)
    rs = eng.resampler(fs, 16000)
    dl = 32 * max(RC.ratio(fs, 16000)) // RC.ratio(fs, 16000)[1]
    assert dl == (64 if fs == 8000 else 32)
    for n in ([0] if N == 1 else [0, 3, 5]):
        yx = rs(x[n])
        assert torch.equal(y16[n, dl:], yx[:256 * K - dl]), (fs, n)
        assert torch.equal(y16[n], rs(torch.cat([torch.zeros(D, device="cuda"), x[n]]))[:256 * K]), (fs, n)


@pytest.mark.parametrize("fs", RC.LIVE_RATES)
def test_pcm16_form_equals_the_float_form_between_the_conversions(eng, win, fs):
    """int16 in, int16 out == f32_to_pcm16(float step(pcm16_to_f32(x))) call by call, and so obeys the identity with u
    rounded to int16."""
    from gtcrn_micro_amd import pcm16_to_f32, f32_to_pcm16
    H, D = GEOM[fs]
    N, K = 3, 12
    gen = torch.Generator(device="cuda").manual_seed(fs)
    x16 = (torch.randn(N, H * K, device="cuda", generator=gen) * 3000).round().clamp(-32768, 32767).to(torch.int16)
    xf = pcm16_to_f32(x16.contiguous())
    sa, sb = eng.new_rate_state(N, win, fs), eng.new_rate_state(N, win, fs)
    o16 = run_stream(eng, sa, x16, [2, 1, 5])
    of = run_stream(eng, sb, xf, [2, 1, 5])
    assert o16.dtype == torch.int16
    assert torch.equal(o16, f32_to_pcm16(of.contiguous()))
    assert torch.equal(sa.rate, sb.rate) and torch.equal(sa.wave, sb.wave) and torch.equal(sa.model, sb.model)
    for n in range(N):
        check_identity(eng, win, fs, of[n], xf[n], f"fs {fs} stream {n}")
    assert o16.any()


def test_many_streams_and_a_drained_tail(eng, win):
    """300 streams at 48 kHz (more than one round of workgroups in every kernel), 5-hop calls; then ceil(latency / H)
    hops of zeros drain the stream: the whole of u comes out."""
    fs = 48000
    H, D = GEOM[fs]
    N, K = 300, 10
    gen = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(N, H * K, device="cuda", generator=gen) * 0.1
    st = eng.new_rate_state(N, win, fs)
    drain = -(-st.latency // H)
    assert drain == 2
    xz = torch.cat([x, torch.zeros(N, H * drain, device="cuda")], 1)
    out = run_stream(eng, st, xz, [5])
    for n in (0, 1, 150, 299):
        check_identity(eng, win, fs, out[n], xz[n], f"stream {n}")
    one = eng.new_rate_state(1, win, fs)
    assert torch.equal(run_stream(eng, one, xz[299:300], [1]), out[299:300])


@pytest.mark.parametrize("fs", [48000, 8000])
def test_rate_step_is_graph_capturable(eng, win, fs):
    """After rate_stream_reserve one rate step captures into a HIP graph (one stream, five launches in a row); replayed
    over 24 hops with new samples copied into the captured buffer it gives the eager run's outputs and states."""
    H, _ = GEOM[fs]
    N, T = 16, 24
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, H * T, device="cuda", generator=gen) * 0.1
    ref_st = eng.new_rate_state(N, win, fs)
    ref = [eng.rate_stream_step(ref_st, x[:, H * t:H * (t + 1)]).clone() for t in range(T)]
    xb = torch.empty(N, H, device="cuda")
    yb = torch.empty(N, H, device="cuda")
    st = eng.new_rate_state(N, win, fs)
    warm = eng.new_rate_state(N, win, fs)
    eng.rate_stream_reserve(st, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        xb.copy_(x[:, :H])
        eng.rate_stream_step(warm, xb, out=yb)                       # warm-up on the capture stream (another state)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            eng.rate_stream_step(st, xb, out=yb)
    eng.rate_stream_reset(st)                                        # the capture itself did not run the step
    torch.cuda.synchronize()
    for t in range(T):
        xb.copy_(x[:, H * t:H * (t + 1)])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yb, ref[t]), t
    assert torch.equal(st.model, ref_st.model)
    assert torch.equal(st.wave, ref_st.wave)
    assert torch.equal(st.rate, ref_st.rate)


def test_stream_wrapper_takes_the_rate_form(eng, win):
    """StreamGTCRNMicro.init_wave_state(..., fs=48000) / step_wave run the rate form; fs=16000 stays the wave form."""
    from gtcrn_micro_amd._lib import RateStreamState
    from gtcrn_micro_amd.streaming.gtcrn_micro_stream import StreamGTCRNMicro
    stream = StreamGTCRNMicro().cuda().eval()
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(2, 768 * 4, device="cuda", generator=gen) * 0.1
    st = stream.init_wave_state(2, win, fs=48000)
    assert isinstance(st, RateStreamState) and st.hop == 768
    got = torch.cat([stream.step_wave(x[:, 768 * k:768 * (k + 1)], st) for k in range(4)], 1)
    e = stream.engine(x.device)
    want = e.rate_stream_step(e.new_rate_state(2, win, 48000), x)
    assert torch.equal(got, want) and got[:, 768:].any()
    assert not isinstance(stream.init_wave_state(2, win), RateStreamState)


def test_bad_arguments_return_err_arg_and_launch_nothing(eng, win):
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import lib, Resampler
    N, fs = 4, 48000
    st = eng.new_rate_state(N, win, fs)
    x = torch.zeros(N, 1536, device="cuda")
    out = torch.full((N, 1536), 7.0, device="cuda")
    for bad_fs in (16000, 44100, 12345):
        with pytest.raises(GtcrnError):
            eng.new_rate_state(N, win, bad_fs)
    for bad in (torch.zeros(N, 1000, device="cuda"), torch.zeros(N + 1, 1536, device="cuda"),
                torch.zeros(N, 1536, device="cuda", dtype=torch.float64), torch.zeros(N, 0, device="cuda")):
        with pytest.raises(GtcrnError):
            eng.rate_stream_step(st, bad, out=out)
    with pytest.raises(GtcrnError):
        eng.rate_stream_step(st, x, out=torch.empty(N, 768, device="cuda"))
    with pytest.raises(GtcrnError):
        eng.rate_stream_step(eng.new_wave_state(N, win), x)
    with pytest.raises(GtcrnError):
        eng.rate_stream_reset(st, 3, 2)
    L, h, sp = lib(), eng._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ri, ro = st.rs_in._h, st.rs_out._h
    r8 = Resampler(8000, 16000, 0)._h
    m, w, r, xi, o, wi = (st.model.data_ptr(), st.wave.data_ptr(), st.rate.data_ptr(), x.data_ptr(), out.data_ptr(),
                          st.window.data_ptr())
    step = L.gtcrn_rate_stream_step
    calls = [
        lambda: step(None, ri, ro, m, w, r, xi, 1536, o, 1536, N, 2, wi, sp),
        lambda: step(h, None, ro, m, w, r, xi, 1536, o, 1536, N, 2, wi, sp),
        lambda: step(h, ri, None, m, w, r, xi, 1536, o, 1536, N, 2, wi, sp),
        lambda: step(h, ro, ri, m, w, r, xi, 1536, o, 1536, N, 2, wi, sp),          # the pair the wrong way round
        lambda: step(h, r8, ro, m, w, r, xi, 1536, o, 1536, N, 2, wi, sp),          # 8 kHz in, 48 kHz out
        lambda: step(h, ri, ro, None, w, r, xi, 1536, o, 1536, N, 2, wi, sp),
        lambda: step(h, ri, ro, m, None, r, xi, 1536, o, 1536, N, 2, wi, sp),
        lambda: step(h, ri, ro, m, w, None, xi, 1536, o, 1536, N, 2, wi, sp),
        lambda: step(h, ri, ro, m, w, r, None, 1536, o, 1536, N, 2, wi, sp),
        lambda: step(h, ri, ro, m, w, r, xi, 1536, None, 1536, N, 2, wi, sp),
        lambda: step(h, ri, ro, m, w, r, xi, 1536, o, 1536, N, 2, None, sp),
        lambda: step(h, ri, ro, m, w, r, xi, 1536, o, 1536, 0, 2, wi, sp),
        lambda: step(h, ri, ro, m, w, r, xi, 1536, o, 1536, N, 0, wi, sp),
        lambda: step(h, ri, ro, m, w, r, xi, 1535, o, 1536, N, 2, wi, sp),
        lambda: step(h, ri, ro, m, w, r, xi, 1536, o, 1000, N, 2, wi, sp),
        lambda: step(h, ri, ro, m, w, r + 4, xi, 1536, o, 1536, N, 2, wi, sp),      # state off the 16-byte grid
        lambda: L.gtcrn_rate_stream_step_pcm16(h, ri, ro, m, w, r, xi, 1536, o, 1536, N, 0, wi, sp),
        lambda: L.gtcrn_rate_stream_reset(h, ri, ro, m, w, None, N, sp),
        lambda: L.gtcrn_rate_stream_reset(h, ri, ro, m, w, r, 0, sp),
        lambda: L.gtcrn_rate_stream_reset(h, ro, ri, m, w, r, N, sp),
        lambda: L.gtcrn_rate_stream_reserve(h, ri, ro, 0, 1),
        lambda: L.gtcrn_rate_stream_reserve(h, ri, r8, N, 1),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i                                          # GTCRN_ERR_ARG
        assert L.gtcrn_last_error(), i
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert not st.wave.any() and not st.rate.any()                   # nothing ran: the states are still reset
