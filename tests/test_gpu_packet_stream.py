"""Packet-sized live streaming (gtcrn_packet_stream_*): one packet of n samples at fs in, n enhanced samples out per stream
and call, at a constant latency, equal to gtcrn_forward_wave (and the batch resamplers around it) bit for bit (contract:
include/gtcrn_micro_hip.h).  Every comparison is exact."""
import ctypes
from math import gcd

import pytest

from conftest import load_params
import resample_checker as RC

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
    return torch.hann_window(512).pow(0.5).cuda()


def run_packets(eng, st, x, resets=None, taps=None):
    """x (N, n C) in C calls of one packet; resets = {call: (lo, hi)}: those streams are reset before that call.  Returns
    the outputs, {call: the group's phase at that reset} and the hops of every call; taps = (list, list) receive the
    16 kHz hand-offs (into / out of the wave step) of the calls that stepped a hop."""
    n, C = st.packet, x.shape[1] // st.packet
    resets = resets or {}
    outs, zs, hops = [], {}, []
    for c in range(C):
        if c in resets:
            zs[c] = st.phase
            eng.packet_stream_reset(st, *resets[c])
        h = st.next_hops
        assert h == (st.phase + st.n16) // 256
        outs.append(eng.packet_stream_step(st, x[:, n * c:n * (c + 1)]))
        hops.append(h)
        if taps is not None and h:
            taps[0].append(eng.packet_stream_handoff(st, 0))
            taps[1].append(eng.packet_stream_handoff(st, 1))
    return torch.cat(outs, 1), zs, hops


def identity_16k(eng, win, a16, z, lat16):
    """What the contract puts out at 16 kHz for a stream that joined at phase z and has taken a16 (1-D) since:
    zeros(L16 - z) ++ gtcrn_forward_wave(zeros(z) ++ a16), cut to len(a16).  Returns (that, the samples of Y in it)."""
    lead = lat16 - z
    assert lead >= 256
    m = a16.numel() - lead
    if m <= 0:
        return torch.zeros_like(a16), 0
    Y = eng.forward_wave(torch.cat([torch.zeros(z, device="cuda"), a16]), win)
    assert Y.dim() == 1 and m <= Y.numel()   # nothing is emitted that the offline call does not have
    return torch.cat([torch.zeros(lead, device="cuda"), Y[:m]]), m


def segments(N, C, resets):
    """{stream: [(first call, end call), ...]} between the resets."""
    starts, segs = {s: 0 for s in range(N)}, {s: [] for s in range(N)}
    for c, (lo, hi) in sorted(resets.items()):
        for s in range(lo, hi):
            segs[s].append((starts[s], c))
            starts[s] = c
    for s in range(N):
        segs[s].append((starts[s], C))
    return segs


def test_hop_sized_packets_equal_the_wave_step(eng, win):
    """16 kHz, n = 256: the calls equal gtcrn_wave_stream_step call by call, outputs and both states."""
    N, K = 5, 12
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(N, 256 * K, device="cuda", generator=gen) * 0.1
    ps, ws = eng.new_packet_state(N, win, 256), eng.new_wave_state(N, win)
    assert ps.latency16 == 256 and ps.period == 1 and ps.n16 == 256
    for k in range(K):
        assert ps.phase == 0 and ps.next_hops == 1
        a = eng.packet_stream_step(ps, x[:, 256 * k:256 * (k + 1)])
        b = eng.wave_stream_step(ws, x[:, 256 * k:256 * (k + 1)])
        assert torch.equal(a, b), k
        assert torch.equal(ps.model, ws.model) and torch.equal(ps.wave, ws.wave), k
    assert a.any() and not ps.pkt.any()      # both FIFOs stay empty


@pytest.mark.parametrize("n", [80, 160, 320, 257, 640, 1000])
@pytest.mark.parametrize("N", [1, 6])
def test_16k_identity_bit_for_bit(eng, win, n, N):
    """At least three periods and 40 hops; with N = 6, streams 1..2 are reset after 3 calls and stream 4 after 7: every
    (stream, segment since its reset) obeys out == zeros(L16 - z) ++ forward_wave(zeros(z) ++ x) with the z of its join."""
    from gtcrn_micro_amd._lib import packet_stream_latency16
    g = gcd(n, 256)
    lat = packet_stream_latency16(16000, n)
    assert lat == 512 - g
    C = max(3 * (256 // g), -(-40 * 256 // n) + 2)
    gen = torch.Generator(device="cuda").manual_seed(n + N)
    x = torch.randn(N, n * C, device="cuda", generator=gen) * 0.1
    st = eng.new_packet_state(N, win, n)
    assert (st.packet, st.n16, st.latency16, st.fs, st.period) == (n, n, lat, 16000, 256 // g)
    resets = {3: (1, 3), 7: (4, 5)} if N > 1 else {}
    out, zs, hops = run_packets(eng, st, x, resets)
    assert out.shape == x.shape and sum(hops) >= 40 and sum(hops) == n * C // 256
    if N > 1:
        assert zs == {3: 3 * n % 256, 7: 7 * n % 256} and all(zs.values())         # joins at z != 0
    checked = 0
    for s, segs in segments(N, C, resets).items():
        for a, b in segs:
            z = zs.get(a, 0)
            want, m = identity_16k(eng, win, x[s, n * a:n * b], z, lat)
            assert torch.equal(out[s, n * a:n * b], want), (n, s, a, b, z)
            checked += m
    assert checked > 0 and out.any()


RATE_CASES = [(8000, 80), (24000, 240), (32000, 320), (48000, 480), (48000, 960), (44100, 441), (22050, 441)]


def stage_reference(eng, win, fs, n, x, z):
    """The contract's chain through the public batch calls for one stream's input x (1-D) since its reset at phase z:
    (a16, out, samples of forward_wave in it, d_in)."""
    from gtcrn_micro_amd._lib import packet_stream_latency16
    up, down, half, _ = RC.design(fs, 16000)
    upo, downo, halfo, _ = RC.design(16000, fs)
    d_in, d_out = half // down, halfo // upo
    calls = x.numel() // n
    n16 = n * 16000 // fs
    c = -(-d_in // up)
    a16 = eng.resampler(fs, 16000)(torch.cat([torch.zeros(c * down, device="cuda"), x]))[c * up - d_in:][:n16 * calls]
    assert a16.numel() == n16 * calls
    b16, m = identity_16k(eng, win, a16, z, packet_stream_latency16(fs, n) - d_in - d_out)
    out = eng.resampler(16000, fs)(torch.cat([torch.zeros(d_out, device="cuda"), b16]))[:n * calls]
    assert out.numel() == n * calls
    return a16, out, m, d_in


@pytest.mark.parametrize("fs,n", RATE_CASES)
def test_rate_identity_stage_by_stage(eng, win, fs, n):
    """Three streams, stream 1 reset after 3 calls.  The 16 kHz samples k_packet_in hands to the wave step are
    gtcrn_resample(fs -> 16k)(x) delayed by d_in (the decimator's pre-ringing in front) behind the z zeros of the join;
    the output is gtcrn_resample(16k -> fs) of zeros(d_out) ++ the 16 kHz identity on them."""
    n16 = n * 16000 // fs
    g = gcd(n16, 256)
    C = max(3 * (256 // g), -(-40 * 256 // n16) + 2)
    N = 3
    gen = torch.Generator(device="cuda").manual_seed(fs + n)
    x = torch.randn(N, n * C, device="cuda", generator=gen) * 0.1
    st = eng.new_packet_state(N, win, n, fs)
    assert st.n16 == n16 and st.rs_in.fs_in == fs and st.rs_out.fs_out == fs
    taps = ([], [])
    out, zs, hops = run_packets(eng, st, x, {3: (1, 2)}, taps)
    assert zs[3] == 3 * n16 % 256 and zs[3] != 0 and sum(hops) >= 40
    hand = torch.cat(taps[0], 1)             # (N, 256 * hops): the hop sequence the model saw
    T = hand.shape[1]
    assert T == 256 * sum(hops)
    for s in (0, 2):                         # never reset: z = 0
        a16, want, m, d_in = stage_reference(eng, win, fs, n, x[s], 0)
        assert m > 0 and torch.equal(out[s], want), (fs, n, s)
        assert torch.equal(hand[s], a16[:T]), (fs, n, s)
        assert torch.equal(hand[s, d_in:], eng.resampler(fs, 16000)(x[s])[:T - d_in]), (fs, n, s)
    _, want, m, _ = stage_reference(eng, win, fs, n, x[1, 3 * n:], zs[3])
    assert m > 0 and torch.equal(out[1, 3 * n:], want), (fs, n, "joined")
    _, want, _, _ = stage_reference(eng, win, fs, n, x[1, :3 * n], 0)
    assert torch.equal(out[1, :3 * n], want), (fs, n, "before the reset")


def test_48k_hop_sized_packets_equal_the_rate_step(eng, win):
    """48 kHz, n = 768 (n16 = 256), z = 0: the calls equal gtcrn_rate_stream_step, outputs and all three states."""
    N, K = 3, 12
    gen = torch.Generator(device="cuda").manual_seed(48)
    x = torch.randn(N, 768 * K, device="cuda", generator=gen) * 0.1
    ps, rs = eng.new_packet_state(N, win, 768, 48000), eng.new_rate_state(N, win, 48000)
    assert ps.latency16 * 3 == rs.latency == 960
    for k in range(K):
        a = eng.packet_stream_step(ps, x[:, 768 * k:768 * (k + 1)])
        b = eng.rate_stream_step(rs, x[:, 768 * k:768 * (k + 1)])
        assert torch.equal(a, b), k
    assert a.any()
    assert torch.equal(ps.model, rs.model) and torch.equal(ps.wave, rs.wave)
    assert torch.equal(ps.pkt[:, 512:], rs.rate) and not ps.pkt[:, :512].any()


@pytest.mark.parametrize("fs,n", [(16000, 160), (48000, 480), (44100, 441), (8000, 80)])
def test_pcm16_form_equals_the_float_form_between_the_conversions(eng, win, fs, n):
    from gtcrn_micro_amd import pcm16_to_f32, f32_to_pcm16
    N, C = 8, 24
    gen = torch.Generator(device="cuda").manual_seed(fs)
    x16 = (torch.randn(N, n * C, device="cuda", generator=gen) * 3000).round().clamp(-32768, 32767).to(torch.int16)
    xf = pcm16_to_f32(x16.contiguous())
    sa, sb = eng.new_packet_state(N, win, n, fs), eng.new_packet_state(N, win, n, fs)
    o16, _, _ = run_packets(eng, sa, x16, {5: (2, 4)})
    of, _, _ = run_packets(eng, sb, xf, {5: (2, 4)})
    assert o16.dtype == torch.int16 and o16.any()
    assert torch.equal(o16, f32_to_pcm16(of.contiguous()))
    assert torch.equal(sa.pkt, sb.pkt) and torch.equal(sa.wave, sb.wave) and torch.equal(sa.model, sb.model)
    assert sa.phase == sb.phase == n * 16000 // fs * C % 256


def test_many_streams_and_a_drained_tail(eng, win):
    """300 streams at 48 kHz in 10 ms packets (more than one round of workgroups in every kernel), then
    ceil(latency / packet) packets of zeros: all of u comes out, and a stream run alone gives the same bits."""
    fs, n = 48000, 480
    N, C = 300, 24
    gen = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(N, n * C, device="cuda", generator=gen) * 0.1
    st = eng.new_packet_state(N, win, n, fs)
    lat_fs = st.latency16 * fs // 16000
    assert st.latency16 == 544 and lat_fs == 1632
    drain = -(-lat_fs // n)
    assert drain == 4
    xz = torch.cat([x, torch.zeros(N, n * drain, device="cuda")], 1)
    out, _, _ = run_packets(eng, st, xz)
    for s in (0, 1, 150, 299):
        _, want, m, _ = stage_reference(eng, win, fs, n, xz[s], 0)
        assert m >= 160 * C and torch.equal(out[s], want), s     # every 16 kHz sample that came from x is out
    one = eng.new_packet_state(1, win, n, fs)
    alone, _, _ = run_packets(eng, one, xz[299:300])
    assert torch.equal(alone, out[299:300])


@pytest.mark.parametrize("fs,n", [(16000, 160), (48000, 480)])
def test_a_whole_period_is_graph_capturable(eng, win, fs, n):
    """One period of 256 / g steps (each with its own packet buffers) captured in one graph and replayed three times
    equals 3 periods of eager calls, outputs and states; a step allocates nothing after new_packet_state."""
    N = 16
    st = eng.new_packet_state(N, win, n, fs)
    P = st.period
    assert P == 8
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, n * P * 3, device="cuda", generator=gen) * 0.1
    ref_st = eng.new_packet_state(N, win, n, fs)
    ref, _, hops = run_packets(eng, ref_st, x)
    assert 0 in hops[:P] and hops[:P] == hops[P:2 * P]
    xb = torch.empty(P, N, n, device="cuda")
    yb = torch.empty(P, N, n, device="cuda")
    warm = eng.new_packet_state(N, win, n, fs)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        xb.copy_(x[:, :n * P].reshape(N, P, n).transpose(0, 1))
        for p in range(P):
            eng.packet_stream_step(warm, xb[p], out=yb[p])             # warm-up on the capture stream (another state)
        torch.cuda.synchronize()
        assert st.phase == 0
        with torch.cuda.graph(g, stream=s):
            for p in range(P):
                eng.packet_stream_step(st, xb[p], out=yb[p])
    assert st.phase == 0                                               # the period closed: the graph may be replayed
    eng.packet_stream_reset(st)                                        # the capture itself did not run the steps
    torch.cuda.synchronize()
    for r in range(3):
        xb.copy_(x[:, n * P * r:n * P * (r + 1)].reshape(N, P, n).transpose(0, 1))
        g.replay()
        torch.cuda.synchronize()
        got = yb.transpose(0, 1).reshape(N, P * n)
        assert torch.equal(got, ref[:, n * P * r:n * P * (r + 1)]), r
    assert torch.equal(st.model, ref_st.model) and torch.equal(st.wave, ref_st.wave) and torch.equal(st.pkt, ref_st.pkt)


def _launches(eng, fn):
    eng.timing_enable(True)
    fn()
    torch.cuda.synchronize()
    t = {k: v[1] for k, v in eng.timing_read().items()}
    eng.timing_enable(False)
    return t


@pytest.mark.parametrize("fs,n", [(16000, 160), (16000, 640), (48000, 480), (44100, 441)])
def test_a_call_is_two_launches_plus_the_wave_step(eng, win, fs, n):
    """From the library's launch records: a call with h = 0 launches k_packet_in and k_packet_out and nothing else; a
    call with h >= 1 those two plus exactly what gtcrn_wave_stream_step launches for h hops.  The resampling stages are
    inside the two kernels: no other kernel runs at any rate."""
    N = 8
    assert "k_packet_in" in eng.kernel_names() and "k_packet_out" in eng.kernel_names()
    st = eng.new_packet_state(N, win, n, fs)
    x = torch.randn(N, n, device="cuda") * 0.1
    y = torch.empty_like(x)
    seen = set()
    for _ in range(st.period):
        h = st.next_hops
        got = _launches(eng, lambda: eng.packet_stream_step(st, x, out=y))
        assert not any(k.startswith("k_rate") or k.startswith("k_resample") for k in got)
        want = {"k_packet_in": 1, "k_packet_out": 1}
        if h:
            ws = eng.new_wave_state(N, win)
            xw = torch.zeros(N, 256 * h, device="cuda")
            wave = _launches(eng, lambda: eng.wave_stream_step(ws, xw))
            assert wave and "k_packet_in" not in wave
            want.update(wave)
        assert got == want, (fs, n, h, got, want)
        seen.add(h)
    assert (0 in seen or n == 640) and max(seen) >= (2 if n == 640 else 1)


def test_stream_wrapper_takes_the_packet_form(eng, win):
    from gtcrn_micro_amd._lib import PacketStreamState
    from gtcrn_micro_amd.streaming.gtcrn_micro_stream import StreamGTCRNMicro
    stream = StreamGTCRNMicro().cuda().eval()
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(2, 441 * 16, device="cuda", generator=gen) * 0.1
    st = stream.init_wave_state(2, win, fs=44100, packet=441)
    assert isinstance(st, PacketStreamState) and st.n16 == 160 and st.latency16 == 544
    got = torch.cat([stream.step_wave(x[:, 441 * k:441 * (k + 1)], st) for k in range(16)], 1)
    e = stream.engine(x.device)
    want, _, _ = run_packets(e, e.new_packet_state(2, win, 441, 44100), x)
    assert torch.equal(got, want) and got.any()
    assert not isinstance(stream.init_wave_state(2, win), PacketStreamState)


def test_bad_arguments_return_err_arg_and_launch_nothing(eng, win):
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import lib
    N, fs, n = 4, 48000, 480
    st = eng.new_packet_state(N, win, n, fs)
    x = torch.zeros(N, n, device="cuda")
    out = torch.full((N, n), 7.0, device="cuda")
    for bad_fs, bad_n in ((11025, 441), (12345, 160), (48000, 100), (16000, 4097), (8000, 40), (22050, 220)):
        with pytest.raises(GtcrnError):
            eng.new_packet_state(N, win, bad_n, bad_fs)
    for bad in (torch.zeros(N, 960, device="cuda"), torch.zeros(N + 1, n, device="cuda"),
                torch.zeros(N, n, device="cuda", dtype=torch.float64), torch.zeros(N, 0, device="cuda")):
        with pytest.raises(GtcrnError):
            eng.packet_stream_step(st, bad, out=out)
    with pytest.raises(GtcrnError):
        eng.packet_stream_step(st, x, out=torch.empty(N, 256, device="cuda"))
    with pytest.raises(GtcrnError):
        eng.packet_stream_step(eng.new_wave_state(N, win), x)
    with pytest.raises(GtcrnError):
        eng.packet_stream_reset(st, 3, 2)
    L, sp = lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ri, ro = st.rs_in._h, st.rs_out._h
    r8 = eng.resampler(8000, 16000)._h
    m, w, p, xi, o, wi = (st.model.data_ptr(), st.wave.data_ptr(), st.pkt.data_ptr(), x.data_ptr(), out.data_ptr(),
                          st.window.data_ptr())
    step, h = L.gtcrn_packet_stream_step, ctypes.c_void_p()
    create = lambda *a: L.gtcrn_packet_stream_create(ctypes.byref(h), *a)      # noqa: E731
    calls = [
        lambda: step(None, m, w, p, xi, n, o, n, N, wi, sp),
        lambda: step(st._h, None, w, p, xi, n, o, n, N, wi, sp),
        lambda: step(st._h, m, None, p, xi, n, o, n, N, wi, sp),
        lambda: step(st._h, m, w, None, xi, n, o, n, N, wi, sp),
        lambda: step(st._h, m, w, p, None, n, o, n, N, wi, sp),
        lambda: step(st._h, m, w, p, xi, n, None, n, N, wi, sp),
        lambda: step(st._h, m, w, p, xi, n, o, n, N, None, sp),
        lambda: step(st._h, m, w, p, xi, n, o, n, 0, wi, sp),
        lambda: step(st._h, m, w, p, xi, n, o, n, N + 1, wi, sp),              # more than max_streams
        lambda: step(st._h, m, w, p, xi, n - 1, o, n, N, wi, sp),
        lambda: step(st._h, m, w, p, xi, n, o, n - 1, N, wi, sp),
        lambda: step(st._h, m, w, p + 4, xi, n, o, n, N, wi, sp),              # state off the 16-byte grid
        lambda: L.gtcrn_packet_stream_step_pcm16(st._h, m, w, p, xi, n, o, n, 0, wi, sp),
        lambda: L.gtcrn_packet_stream_reset(st._h, m, w, None, N, sp),
        lambda: L.gtcrn_packet_stream_reset(st._h, m, w, p, 0, sp),
        lambda: L.gtcrn_packet_stream_reset(st._h, m, w, p, N + 1, sp),
        lambda: create(eng._h, ro, ri, fs, n, N),                              # the pair the wrong way round
        lambda: create(eng._h, r8, ro, fs, n, N),                              # 8 kHz in, 48 kHz out
        lambda: create(eng._h, None, ro, fs, n, N),
        lambda: create(eng._h, ri, ro, 16000, 160, N),                         # 16 kHz takes no resamplers
        lambda: create(eng._h, ri, ro, fs, n, 0),
        lambda: create(eng._h, ri, ro, fs, 100, N),
        lambda: create(None, ri, ro, fs, n, N),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i                                          # GTCRN_ERR_ARG
        assert L.gtcrn_last_error(), i
        assert not h.value, i
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert not st.wave.any() and not st.pkt.any() and st.phase == 0  # nothing ran: the states are still reset
