"""The high band on the GPU (gtcrn_rate_stream_step_hb / gtcrn_resample_hb; contract: include/gtcrn_micro_hip.h, "high
band"): the exact bypass, gamma = 0 against the plain and the limited step, the live contract against
tests/highband_checker.py, a tone above the band, chunking, a sub-range reset, a captured step that follows new gains, the
offline form and the argument errors."""
import numpy as np
import pytest

from conftest import load_params
import highband_checker as HC
import resample_checker as RC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 3
HB_RATES = (24000, 32000, 48000)
GEOM = {24000: (384, 48), 32000: (512, 64), 48000: (768, 96)}      # fs: (H, D)


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


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def noise(fs, K, seed, scale=0.1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(N, GEOM[fs][0] * K, device="cuda", generator=gen) * scale


def run(eng, st, x, chunks, taps=None):
    """x (N, H K) through the state in calls of `chunks` hops; taps: a list that receives (a, w) of every call."""
    H, k, outs = st.hop, 0, []
    for nh in chunks:
        outs.append(eng.rate_stream_step(st, x[:, H * k:H * (k + nh)]))
        if taps is not None:
            taps.append((eng.rate_stream_handoff(st, nh, 0), eng.rate_stream_handoff(st, nh, 1)))
        k += nh
    assert H * k == x.shape[1]
    return torch.cat(outs, 1)


def states(st):
    return [st.model, st.wave, st.rate] + ([st.hb] if st.hb is not None else [])


# ------------------------------------------------------------------------------------------------ 1. the exact bypass
@pytest.mark.parametrize("fs", HB_RATES)
@pytest.mark.parametrize("chunks", [(1, 1, 1, 1), (2, 2)])
@pytest.mark.parametrize("pcm", [False, True])
def test_bypass_is_exact(eng, win, fs, chunks, pcm):
    """atten_lim_db = 0 and highband = 1: out == zeros(LAT) ++ x, bit for bit.  One hop per call has H < LAT (the delay line
    shifts); two hops per call read the delayed input from the call's own rows."""
    x = noise(fs, 4, fs + 1, 0.3)
    if pcm:
        x = (x * 20000).round().clamp(-32768, 32767).to(torch.int16)
    st = eng.new_rate_state(N, win, fs, atten_lim_db=0, highband=1.0)
    out = run(eng, st, x, chunks)
    lat = st.latency
    assert lat == GEOM[fs][0] + 2 * GEOM[fs][1] and out.dtype == x.dtype
    want = torch.cat([torch.zeros(N, lat, device="cuda", dtype=x.dtype), x], 1)[:, :x.shape[1]]
    assert torch.equal(out, want), int((out != want).sum())
    assert out[:, lat:].any()


# ------------------------------------------------------------------------------------------------ 2. gamma = 0
@pytest.mark.parametrize("fs", HB_RATES)
@pytest.mark.parametrize("lim", [None, 12.0])
@pytest.mark.parametrize("pcm", [False, True])
def test_gain_zero_equals_the_plain_and_the_limited_step(eng, win, fs, lim, pcm):
    x = noise(fs, 5, fs + 2)
    if pcm:
        x = (x * 30000).round().clamp(-32768, 32767).to(torch.int16)
    ref = eng.new_rate_state(N, win, fs, atten_lim_db=lim)
    st = eng.new_rate_state(N, win, fs, atten_lim_db=lim, highband=0.0)
    want = run(eng, ref, x, (2, 1, 2))
    got = run(eng, st, x, (2, 1, 2))
    assert torch.equal(got, want) and got.any()                    # (==: a zero may differ in sign)
    for a, b in zip(states(ref), states(st)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. the contract
@pytest.mark.parametrize("fs", HB_RATES)
@pytest.mark.parametrize("lim", [None, 12.0])
def test_live_contract_against_the_checker(eng, win, fs, lim):
    """Per-stream gains (0.25, 0.5, 1.0); a and w are the 16 kHz hand-offs of the calls themselves.  Tolerance: the fp32
    dot-product bound of tests/test_gpu_resample.py for the outbound stage ((n + 1) 2^-24 sum |s_i| |h_k|, times 1 + 2^-26
    for the float64 reference) plus two fp32 roundings of the mix, 2 * 2^-24 (|v| + |gamma x|)."""
    from gtcrn_micro_amd._lib import resample_taps
    up, down, h = resample_taps(16000, fs)
    gains = (0.25, 0.5, 1.0)
    x = noise(fs, 6, fs + 3)
    st = eng.new_rate_state(N, win, fs, atten_lim_db=lim, highband=gains)
    taps = []
    out = run(eng, st, x, (1, 2, 1, 2), taps).cpu().numpy().astype(np.float64)
    a = torch.cat([t[0] for t in taps], 1).cpu().numpy()
    w = torch.cat([t[1] for t in taps], 1).cpu().numpy()
    xs = x.cpu().numpy()
    worst = 0.0
    for n in range(N):
        r = HC.live(a[n], w[n], xs[n], gains[n], up, down, h)
        err = np.abs(out[n] - r["out"])
        nz = r["bound"] > 0
        worst = max(worst, float((err[nz] / r["bound"][nz]).max()))
        assert (err <= r["bound"]).all(), (fs, lim, n, float((err - r["bound"]).max()))
        assert np.abs(r["dry"]).max() > 0.01 and np.abs(r["v"]).max() > 1e-3      # both terms are in play
    print(f"fs {fs} limit {lim}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 4. a tone above the band
def _tone_amplitude(y, f, fs, start):
    seg = y[start:].astype(np.float64)
    n = np.arange(seg.size)
    wnd = np.hanning(seg.size)
    return 2 * abs(np.sum(seg * wnd * np.exp(-2j * np.pi * f * n / fs))) / wnd.sum()


@pytest.mark.parametrize("fs,f", [(48000, 12000.0), (24000, 10000.0)])
def test_a_tone_above_the_band_survives(eng, win, fs, f):
    """A tone of amplitude 0.25 above 9 kHz plus noise below 8 kHz, gamma = 0.5: after LAT plus one filter length the
    output's projection on the tone has amplitude 0.125 +- 1e-3 (both stages are >= 96 dB down at the tone: the model path
    contributes < 1e-5); the plain step leaves < 1e-4 of it."""
    H, D = GEOM[fs]
    K = 8
    upo, downo, _, ho = RC.design(16000, fs)
    rng = np.random.default_rng(fs)
    low = RC.resample64(rng.standard_normal((N, 256 * K)) * 0.05, upo, downo, ho)       # nothing above 9 kHz
    n = np.arange(H * K)
    x = cu((low + 0.25 * np.sin(2 * np.pi * f * n / fs + 0.3)).astype(np.float32))
    hb = run(eng, eng.new_rate_state(N, win, fs, highband=0.5), x, (2,) * (K // 2)).cpu().numpy()
    plain = run(eng, eng.new_rate_state(N, win, fs), x, (2,) * (K // 2)).cpu().numpy()
    start = H + 2 * D + len(ho)                                    # (193 taps on the 48 kHz grid: no longer at either fs)
    for s in range(N):
        got, base = _tone_amplitude(hb[s], f, fs, start), _tone_amplitude(plain[s], f, fs, start)
        print(f"fs {fs} stream {s}: tone amplitude {got:.6f} with the high band, {base:.2e} without")
        assert abs(got - 0.125) <= 1e-3, (fs, s, got)
        assert base < 1e-4, (fs, s, base)


# ------------------------------------------------------------------------------------------------ 5. chunking
@pytest.mark.parametrize("fs", HB_RATES)
@pytest.mark.parametrize("pcm", [False, True])
def test_output_and_states_do_not_depend_on_the_chunking(eng, win, fs, pcm):
    x = noise(fs, 4, fs + 5)
    if pcm:
        x = (x * 30000).round().clamp(-32768, 32767).to(torch.int16)
    runs = []
    for chunks in ((4,), (1, 1, 1, 1), (2, 1, 1)):
        st = eng.new_rate_state(N, win, fs, atten_lim_db=6.0, highband=(0.3, 0.7, 1.0))
        runs.append((run(eng, st, x, chunks), st))
    for out, st in runs[1:]:
        assert torch.equal(out, runs[0][0])
        for a, b in zip(states(st), states(runs[0][1])):
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert len(states(runs[0][1])) == 4 and runs[0][1].hb.any()


# ------------------------------------------------------------------------------------------------ 6. sub-range reset
def test_sub_range_reset(eng, win):
    fs = 48000
    H = GEOM[fs][0]
    x = noise(fs, 4, 77)
    gains = (0.25, 0.5, 1.0)
    st = eng.new_rate_state(N, win, fs, highband=gains)
    ref = eng.new_rate_state(N, win, fs, highband=gains)
    first = run(eng, st, x[:, :2 * H], (1, 1))
    eng.rate_stream_reset(st, 1, 2)
    assert not st.hb[1].any() and not st.rate[1].any() and st.hb[0].any() and st.hb[2].any()
    second = run(eng, st, x[:, 2 * H:], (1, 1))
    whole = run(eng, ref, x, (1, 1, 1, 1))
    got = torch.cat([first, second], 1)
    assert torch.equal(got[0], whole[0]) and torch.equal(got[2], whole[2])
    fresh = eng.new_rate_state(N, win, fs, highband=gains)         # stream 1 of a state that starts at hop 2
    alone = run(eng, fresh, x[:, 2 * H:], (1, 1))
    assert torch.equal(second[1], alone[1]) and not torch.equal(second[1], whole[1, 2 * H:])
    for a, b, c in zip(states(st), states(ref), states(fresh)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[1], c[1])


# ------------------------------------------------------------------------------------------------ 7. graph
def test_captured_step_follows_new_gains(eng, win):
    fs = 48000
    H, T = GEOM[fs][0], 6
    x = noise(fs, T, 5)
    g0, g1 = (0.25, 0.5, 1.0), (1.0, 0.0, 0.5)
    ref_st = eng.new_rate_state(N, win, fs, highband=g0)
    ref = []
    for t in range(T):
        if t == 3:
            ref_st.set_highband_gain(g1)
        ref.append(eng.rate_stream_step(ref_st, x[:, H * t:H * (t + 1)]).clone())
    same = eng.new_rate_state(N, win, fs, highband=g0)             # the gains matter: without the change hop 3 differs
    for t in range(4):
        last = eng.rate_stream_step(same, x[:, H * t:H * (t + 1)])
    assert not torch.equal(last, ref[3])
    xb, yb = torch.empty(N, H, device="cuda"), torch.empty(N, H, device="cuda")
    st = eng.new_rate_state(N, win, fs, highband=g0)
    warm = eng.new_rate_state(N, win, fs, highband=g0)
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
        if t == 3:
            st.set_highband_gain(g1)
        xb.copy_(x[:, H * t:H * (t + 1)])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yb, ref[t]), t
    for a, b in zip(states(st), states(ref_st)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 8. offline
def test_offline_form(eng, win):
    """forward_wave_rate(x, 48000, win, out_fs=48000, highband=gamma) at B = 3, unequal lengths (1535 is no multiple of 3 and
    its output, 1536 samples, is one longer than the clip: that sample gets no dry term) against the three public calls
    plus the stated mix in numpy float32, the outbound stage in float64; tolerance as in the live contract test."""
    from gtcrn_micro_amd._lib import resample_taps
    fs = 48000
    up, down, h = resample_taps(16000, fs)
    lengths = [4801, 1535, 3000]
    L = max(lengths)
    gen = torch.Generator(device="cuda").manual_seed(8)
    x = torch.randn(3, L, device="cuda", generator=gen) * 0.1
    gains = (0.25, 0.5, 1.0)
    got = eng.forward_wave_rate(x, fs, win, out_fs=fs, highband=cu(np.array(gains, np.float32)), lengths=lengths)
    rs_in = eng.resampler(fs, 16000)
    l16 = [rs_in.out_len(v) for v in lengths]
    x16 = torch.zeros(3, rs_in.out_len(L), device="cuda")
    rs_in(x, lengths=lengths, out=x16)
    y = eng.forward_wave_var(x16, l16, win).cpu().numpy()
    x16n, xn, gotn = x16.cpu().numpy(), x.cpu().numpy(), got.cpu().numpy()
    assert gotn.shape == (3, 256 * (l16[0] // 256) * 3)
    for b in range(3):
        g = np.float32(gains[b])
        ly = 256 * (l16[b] // 256)
        s = (y[b, :ly] - (g * x16n[b, :ly]).astype(np.float32)).astype(np.float32)
        v = RC.resample64(s, up, down, h)
        nb, nd = v.size, min(v.size, lengths[b])
        assert nb == 3 * ly
        dry = np.zeros(nb, np.float32)
        dry[:nd] = (g * xn[b, :nd]).astype(np.float32)
        bound = RC.dot_bound(s, up, down, h) * (1 + 2.0 ** -26) + 2 * 2.0 ** -24 * (np.abs(v) + np.abs(dry))
        err = np.abs(gotn[b, :nb].astype(np.float64) - (v + dry))
        assert (err <= bound).all(), (b, float((err - bound).max()))
        assert not gotn[b, nb:].any()                                 # nothing behind the row's outputs
    assert 3 * 256 * (l16[1] // 256) == lengths[1] + 1               # the row with a tail past its clip
    # dry_gain = 1 and gamma = 1: the input comes back exactly
    back = eng.forward_wave_rate(x, fs, win, out_fs=fs, dry_gain=1.0, highband=1.0, lengths=lengths)
    for b in range(3):
        nd = min(3 * 256 * (l16[b] // 256), lengths[b])
        assert torch.equal(back[b, :nd], x[b, :nd]), b
    one = eng.forward_wave_rate(x[0], fs, win, out_fs=fs, dry_gain=1.0, highband=1.0)
    assert one.dim() == 1 and torch.equal(one, x[0, :one.numel()]) and one.numel() == 3 * 256 * (l16[0] // 256)


# ------------------------------------------------------------------------------------------------ 9. errors
def test_errors(eng, win):
    from gtcrn_micro_amd import GtcrnError
    for fs in (8000, 44100, 16000):
        with pytest.raises(GtcrnError):
            eng.new_rate_state(N, win, fs, highband=0.5)
    with pytest.raises(GtcrnError):
        eng.new_rate_state(N, win, 48000, highband=1.5)
    with pytest.raises(GtcrnError):
        eng.new_rate_state(N, win, 48000).set_highband_gain(0.5)   # a state without a high band
    st = eng.new_rate_state(N, win, 48000, highband=0.5)
    buf = torch.zeros(N, 768 * 3, device="cuda")
    before = [t.clone() for t in states(st)]
    with pytest.raises(GtcrnError):
        eng.rate_stream_step(st, buf[:, :768], out=buf[:, :768])              # in place
    with pytest.raises(GtcrnError):
        eng.rate_stream_step(st, buf[:, :1536], out=buf[:, 768:2304])         # rows that share a hop
    eng.rate_stream_step(st, buf[:, :768], out=buf[:, 768:1536])              # rows side by side in one buffer are legal
    eng.rate_stream_reset(st)
    torch.cuda.synchronize()
    for a, b in zip(states(st), before):
        assert torch.equal(a, b)
    x = torch.zeros(2, 4800, device="cuda")
    for fs, out_fs in ((48000, None), (48000, 16000), (48000, 24000), (16000, 16000), (8000, 8000), (44100, 44100)):
        with pytest.raises(GtcrnError):
            eng.forward_wave_rate(x, fs, win, out_fs=out_fs, highband=0.5)
    with pytest.raises(GtcrnError):
        eng.forward_wave_rate(x, 48000, win, out_fs=48000, lengths=[4800, 4000])  # lengths= without highband=
