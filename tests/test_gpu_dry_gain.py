"""The attenuation limit (per-stream dry / wet mix, include/gtcrn_micro_hip.h "attenuation limit") on every waveform
path.  The checker is the contract's formula in numpy float32,
    y = fl(fl(beta x) + fl(fl(1 - beta) w)),
applied to the outputs of the plain calls (which the other test files pin) and the inputs.  Every comparison is exact
except the one spectral-equivalence test, which uses the project's 1e-4 relative bound."""
from math import gcd

import numpy as np
import pytest

from conftest import load_params
import resample_checker as RC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

G6, G12 = 10.0 ** (-6 / 20), 10.0 ** (-12 / 20)
GAINS = [0.0, 1.0, G6, G12, 0.3718]            # no limit, bypass, 6 dB, 12 dB, "a random value"
RATE_GEOM = {8000: (128, 32), 48000: (768, 96)}      # fs: (H, D)


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


def gains_for(B, shift=0):
    return torch.tensor([GAINS[(b + shift) % len(GAINS)] for b in range(B)], dtype=torch.float32, device="cuda")


def mix_np(beta, x, w):
    """The formula, numpy float32: beta (B,) or scalar, x and w (B, n) or (n,) tensors -> a CUDA tensor like w."""
    b = np.asarray(beta.cpu().numpy() if isinstance(beta, torch.Tensor) else beta, np.float32)
    if b.ndim == 1 and w.dim() == 2:
        b = b[:, None]
    xn, wn = x.cpu().numpy().astype(np.float32), w.cpu().numpy().astype(np.float32)
    one = np.float32(1)
    y = (b * xn).astype(np.float32) + ((one - b).astype(np.float32) * wn).astype(np.float32)
    return torch.from_numpy(y.astype(np.float32)).to(w.device)


def limited_offline(eng, win, x, g):
    """The reference for every streaming form: formula(plain forward_wave, input), for one clip (1-D) or a batch."""
    w = eng.forward_wave(x, win)
    return mix_np(g, x[..., :w.shape[-1]], w)


def _launches(eng, fn):
    eng.timing_enable(True)
    fn()
    torch.cuda.synchronize()
    t = {k: v[1] for k, v in eng.timing_read().items()}
    eng.timing_enable(False)
    return t


# ------------------------------------------------------------------------------------------------------- 1. offline
@pytest.mark.parametrize("B", [1, 3, 256, 257])
@pytest.mark.parametrize("L", [256 * 9, 256 * 9 + 77])
def test_offline_equals_the_formula(eng, win, B, L):
    gen = torch.Generator(device="cuda").manual_seed(B + L)
    x = torch.randn(B, L, device="cuda", generator=gen) * 0.1
    n = 256 * (L // 256)
    plain = eng.forward_wave(x, win)
    for shift in (range(len(GAINS)) if B == 1 else (B % 3,)):
        g = gains_for(B, shift)
        got = eng.forward_wave(x, win, dry_gain=g)
        assert got.shape == plain.shape == (B, n)
        assert torch.equal(got, mix_np(g, x[:, :n], plain)), (B, L, shift)
        gz, go = (g == 0).nonzero().flatten(), (g == 1).nonzero().flatten()
        assert torch.equal(got[gz], plain[gz]) and torch.equal(got[go], x[go, :n])
        if B > 1:
            assert len(gz) and len(go)
    # one float for the whole batch; a 1-D clip
    assert torch.equal(eng.forward_wave(x, win, dry_gain=G6), mix_np(np.float32(G6), x[:, :n], plain))
    assert torch.equal(eng.forward_wave(x[0], win, dry_gain=1.0), x[0, :n])
    assert torch.equal(eng.forward_wave(x[0], win, dry_gain=0.0), plain[0])


@pytest.mark.parametrize("B", [1, 3, 256, 257])
def test_offline_var_equals_the_formula_and_leaves_the_rest_alone(eng, win, B):
    Lmax = 256 * 11 + 100
    rng = np.random.default_rng(B)
    lens = rng.integers(257, Lmax + 1, B)
    lens[0] = Lmax
    if B > 2:
        lens[1], lens[2] = 512, 257
    gen = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn(B, Lmax, device="cuda", generator=gen) * 0.1
    g = gains_for(B, 1)
    n = 256 * (Lmax // 256)
    plain = eng.forward_wave_var(x, lens, win, out=torch.full((B, n), 7.0, device="cuda"))
    got = eng.forward_wave_var(x, lens, win, out=torch.full((B, n), 7.0, device="cuda"), dry_gain=g)
    want = mix_np(g, x[:, :n], plain)
    for b in range(B):
        nb = 256 * (int(lens[b]) // 256)
        assert torch.equal(got[b, :nb], want[b, :nb]), (B, b)
        assert (got[b, nb:] == 7.0).all() and (plain[b, nb:] == 7.0).all(), (B, b)      # beyond its length: untouched
        if float(g[b]) == 0.0:
            assert torch.equal(got[b, :nb], plain[b, :nb])
        if float(g[b]) == 1.0:
            assert torch.equal(got[b, :nb], x[b, :nb])
    # a row of the batch is the clip alone
    b = B - 1
    alone = eng.forward_wave(x[b, :int(lens[b])], win, dry_gain=float(g[b]))
    assert torch.equal(got[b, :alone.numel()], alone)


def test_gains_outside_the_unit_interval_are_rejected(eng, win):
    from gtcrn_micro_amd import GtcrnError
    x = torch.zeros(2, 1024, device="cuda")
    for bad in (1.5, -0.25, torch.tensor([0.5, 1.5], device="cuda"), torch.tensor([0.5], device="cuda"),
                torch.tensor([0.5, 0.5]), torch.tensor([0.5, float("nan")], device="cuda")):
        with pytest.raises(GtcrnError):
            eng.forward_wave(x, win, dry_gain=bad)


# ------------------------------------------------------------------------------------------------------ 2. hop form
def run_hops(eng, st, x, chunks, plain=None, resets=None):
    """x (N, 256 K) through wave_stream_step in calls of `chunks` hops (cycled); resets {hop: (lo, hi)} reset those
    streams (of both states) before the call that starts there.  plain: a state without the limit stepped alongside; after
    every call both of its states must equal the limited one's."""
    K, outs, k, i = x.shape[1] // 256, [], 0, 0
    resets = resets or {}
    while k < K:
        if k in resets:
            eng.wave_stream_reset(st, *resets[k])
            if plain is not None:
                eng.wave_stream_reset(plain, *resets[k])
        nh = min(chunks[i % len(chunks)], K - k, min([r for r in resets if r > k] + [K]) - k)
        outs.append(eng.wave_stream_step(st, x[:, 256 * k:256 * (k + nh)]))
        if plain is not None:
            eng.wave_stream_step(plain, x[:, 256 * k:256 * (k + nh)])
            assert torch.equal(st.wave, plain.wave) and torch.equal(st.model, plain.model), k
        k += nh
        i += 1
    return torch.cat(outs, 1)


@pytest.mark.parametrize("chunks", [[1], [2], [5], [1, 2, 5]])
def test_hop_stream_is_the_limited_offline_call_one_hop_late(eng, win, chunks):
    """Six streams with mixed limits; streams 1..2 restart at hop 6, stream 4 at hop 11 (the streams of a call sit at
    different hop counts).  Every (stream, segment) is zeros(256) ++ limited offline call; the states follow the plain form."""
    N, K = 6, 21
    gen = torch.Generator(device="cuda").manual_seed(sum(chunks))
    x = torch.randn(N, 256 * K, device="cuda", generator=gen) * 0.1
    db = [None, 0, 6, 12, 8.59, float("inf")]
    st = eng.new_wave_state(N, win, atten_lim_db=db)
    g = st.dry_gain
    assert g.dtype == torch.float32 and g.shape == (N,)
    assert g.tolist() == [0.0, 1.0, np.float32(G6), np.float32(G12), np.float32(10 ** (-8.59 / 20)), 0.0]
    resets = {6: (1, 3), 11: (4, 5)}
    out = run_hops(eng, st, x, chunks, eng.new_wave_state(N, win), resets)
    segs = {s: [(0, K)] for s in range(N)}
    segs[1] = segs[2] = [(0, 6), (6, K)]
    segs[4] = [(0, 11), (11, K)]
    for s in range(N):
        for a, b in segs[s]:
            o = out[s, 256 * a:256 * b]
            assert not o[:256].any(), (s, a)
            want = limited_offline(eng, win, x[s, 256 * a:256 * b], g[s:s + 1])
            assert torch.equal(o[256:], want[:256 * (b - a - 1)]), (chunks, s, a, b)
    assert torch.equal(out[1, 256 * 7:], x[1, 256 * 6:256 * (K - 1)])            # bypass: the input, one hop late
    plain = run_hops(eng, eng.new_wave_state(N, win), x, chunks, None, resets)
    assert torch.equal(out[0], plain[0]) and torch.equal(out[5], plain[5])        # no limit: the plain stream
    assert not torch.equal(out[2], plain[2])


@pytest.mark.parametrize("r", [0, 1, 255])
@pytest.mark.parametrize("nh", [1, 2, 5])
def test_steps_and_flush_give_the_limited_offline_call(eng, win, r, nh):
    N, K = 5, 10
    gen = torch.Generator(device="cuda").manual_seed(r + nh)
    x = torch.randn(N, 256 * K + r, device="cuda", generator=gen) * 0.1
    g = gains_for(N, 2)
    st, plain = eng.new_wave_state(N, win), eng.new_wave_state(N, win)
    st.set_dry_gain(g)
    out = run_hops(eng, st, x[:, :256 * K], [nh], plain)
    last = eng.wave_stream_flush(st, x[:, 256 * K:])
    eng.wave_stream_flush(plain, x[:, 256 * K:])
    assert torch.equal(st.wave, plain.wave) and torch.equal(st.model, plain.model)
    whole = torch.cat([out, last], 1)
    assert whole.shape == (N, 256 * (K + 1)) and not whole[:, :256].any()
    assert torch.equal(whole[:, 256:], limited_offline(eng, win, x, g))


def test_flush_of_a_short_stream_stays_zero(eng, win):
    """Fewer than 257 samples: the flush has no block, also in bypass."""
    N = 3
    st = eng.new_wave_state(N, win, atten_lim_db=0)
    x = torch.randn(N, 256, device="cuda") * 0.1 + 0.5
    assert not eng.wave_stream_step(st, x).any()                                   # the first block of a stream
    assert not eng.wave_stream_flush(st, x[:, :0]).any()                           # 256 samples in all: no block
    st2 = eng.new_wave_state(N, win, atten_lim_db=0)
    assert not eng.wave_stream_flush(st2, x[:, :200]).any()


@pytest.mark.parametrize("nh", [1, 2, 5])
def test_pcm16_form_equals_the_float_form_between_the_conversions(eng, win, nh):
    """The mix is made in float before the ONE rounding to int16."""
    from gtcrn_micro_amd import pcm16_to_f32, f32_to_pcm16
    N, K, r = 5, 10, 96
    gen = torch.Generator(device="cuda").manual_seed(nh)
    x16 = (torch.randn(N, 256 * K + r, device="cuda", generator=gen) * 3000).round().clamp(-32768, 32767).to(torch.int16)
    xf = pcm16_to_f32(x16.contiguous())
    g = gains_for(N, 1)
    assert float(g[0]) == 1.0
    sa, sb, sp = eng.new_wave_state(N, win), eng.new_wave_state(N, win), eng.new_wave_state(N, win)
    sa.set_dry_gain(g)
    sb.set_dry_gain(g)
    o16 = torch.cat([run_hops(eng, sa, x16[:, :256 * K], [nh], sp), eng.wave_stream_flush(sa, x16[:, 256 * K:])], 1)
    of = torch.cat([run_hops(eng, sb, xf[:, :256 * K], [nh]), eng.wave_stream_flush(sb, xf[:, 256 * K:])], 1)
    assert o16.dtype == torch.int16 and o16.any()
    assert torch.equal(o16, f32_to_pcm16(of.contiguous()))
    assert torch.equal(sa.wave, sb.wave) and torch.equal(sa.model, sb.model)
    assert torch.equal(o16[0, 256:256 * K], x16[0, :256 * (K - 1)])               # bypass returns the very int16 samples


# ------------------------------------------------------------------------------------------------------ 3. rate form
@pytest.mark.parametrize("fs", [8000, 48000])
def test_rate_form_mixes_at_16k(eng, win, fs):
    H, D = RATE_GEOM[fs]
    N, K = 4, 14
    gen = torch.Generator(device="cuda").manual_seed(fs)
    x = torch.randn(N, H * K, device="cuda", generator=gen) * 0.1
    st = eng.new_rate_state(N, win, fs, atten_lim_db=[6, 0, None, 12])
    plain = eng.new_rate_state(N, win, fs)
    g = st.dry_gain
    up, _, half, _ = RC.design(fs, 16000)
    ntp_in = (2 * half // up + 1 + 3) // 4 * 4                # the inbound stage's history, in front of the outbound one
    assert 0 < ntp_in < st.rate.shape[1]
    outs, a16, b16, k = [], [], [], 0
    for nh in [1, 2, 5, 1, 2, 3]:
        outs.append(eng.rate_stream_step(st, x[:, H * k:H * (k + nh)]))
        a16.append(eng.rate_stream_handoff(st, nh, 0))
        b16.append(eng.rate_stream_handoff(st, nh, 1))
        eng.rate_stream_step(plain, x[:, H * k:H * (k + nh)])
        assert torch.equal(st.wave, plain.wave) and torch.equal(st.model, plain.model)
        assert torch.equal(st.rate[:, :ntp_in], plain.rate[:, :ntp_in])      # (the outbound history holds emitted samples)
        k += nh
    assert k == K
    out, a16, b16 = torch.cat(outs, 1), torch.cat(a16, 1), torch.cat(b16, 1)
    # the 16 kHz hand-offs satisfy the 16 kHz limited contract
    assert not b16[:, :256].any()
    assert torch.equal(b16[:, 256:], limited_offline(eng, win, a16, g)[:, :256 * (K - 1)])
    # the output: the public batch calls composed, with the limited offline call in the middle
    rs_in, rs_out = eng.resampler(fs, 16000), eng.resampler(16000, fs)
    for s in range(N):
        xd = torch.cat([torch.zeros(D, device="cuda"), x[s]])
        u = eng.forward_wave_rate(xd, fs, win, out_fs=fs, dry_gain=float(g[s]))
        x16 = rs_in(xd)
        assert torch.equal(u, rs_out(limited_offline(eng, win, x16, g[s:s + 1])))
        assert not out[s, :H].any()
        assert torch.equal(out[s, H + D:], u[:H * K - H - D]), (fs, s)
    # bypass: the band-limited input delayed by the form's latency -- the identity in place of the model
    x16 = rs_in(torch.cat([torch.zeros(D, device="cuda"), x[1]]))
    ident = rs_out(x16[:256 * (x16.numel() // 256)])
    assert torch.equal(out[1, H + D:], ident[:H * K - H - D])
    from gtcrn_micro_amd._lib import rate_stream_latency
    assert rate_stream_latency(fs) == H + 2 * D


# ---------------------------------------------------------------------------------------------------- 4. packet form
def run_packets(eng, st, x, resets=None, taps=None, before=None):
    """x (N, n C) in C calls of one packet; resets {call: (lo, hi)}; before {call: callable} runs ahead of that call.
    Returns the outputs, {call: phase at that reset}, the hops of every call."""
    n, C = st.packet, x.shape[1] // st.packet
    resets, before = resets or {}, before or {}
    outs, zs, hops = [], {}, []
    for c in range(C):
        if c in before:
            before[c]()
        if c in resets:
            zs[c] = st.phase
            eng.packet_stream_reset(st, *resets[c])
        hops.append(st.next_hops)
        outs.append(eng.packet_stream_step(st, x[:, n * c:n * (c + 1)]))
        if taps is not None and hops[-1]:
            taps.append(eng.packet_stream_handoff(st, 0))
    return torch.cat(outs, 1), zs, hops


def identity_16k(eng, win, a16, z, lat16, g):
    """The header's 16 kHz contract with Y the limited offline result: zeros(L16 - z) ++ Y(zeros(z) ++ a16), cut."""
    lead = lat16 - z
    m = a16.numel() - lead
    assert lead >= 256 and m > 0
    Y = limited_offline(eng, win, torch.cat([torch.zeros(z, device="cuda"), a16]), g)
    assert m <= Y.numel()
    return torch.cat([torch.zeros(lead, device="cuda"), Y[:m]]), lead


def packet_reference(eng, win, fs, n, x, z, g):
    """The header's chain through the public batch calls for one stream's input x since its reset at phase z."""
    from gtcrn_micro_amd._lib import packet_stream_latency16
    calls, n16 = x.numel() // n, n * 16000 // fs
    if fs == 16000:
        return identity_16k(eng, win, x, z, packet_stream_latency16(fs, n), g)
    up, down, half, _ = RC.design(fs, 16000)
    upo, _, halfo, _ = RC.design(16000, fs)
    d_in, d_out = half // down, halfo // upo
    c = -(-d_in // up)
    a16 = eng.resampler(fs, 16000)(torch.cat([torch.zeros(c * down, device="cuda"), x]))[c * up - d_in:][:n16 * calls]
    b16, lead = identity_16k(eng, win, a16, z, packet_stream_latency16(fs, n) - d_in - d_out, g)
    out = eng.resampler(16000, fs)(torch.cat([torch.zeros(d_out, device="cuda"), b16]))[:n * calls]
    return out, lead * fs // 16000


@pytest.mark.parametrize("fs,n", [(16000, 160), (16000, 320), (48000, 480), (44100, 441)])
def test_packet_form_holds_its_contract_with_the_limited_offline_call(eng, win, fs, n):
    """Three periods; stream 1 is reset before call 3, at a phase z != 0.  The pre-fill stays zero, also in bypass."""
    n16 = n * 16000 // fs
    P = 256 // gcd(n16, 256)
    C = max(3 * P, -(-30 * 256 // n16) + 2)
    N = 4
    gen = torch.Generator(device="cuda").manual_seed(fs + n)
    x = torch.randn(N, n * C, device="cuda", generator=gen) * 0.1 + 0.01
    st = eng.new_packet_state(N, win, n, fs, atten_lim_db=[12, 0, 6, None])
    plain = eng.new_packet_state(N, win, n, fs)
    g = st.dry_gain
    out, zs, hops = run_packets(eng, st, x, {3: (1, 2)})
    outp, _, _ = run_packets(eng, plain, x, {3: (1, 2)})
    assert C >= 2 * P and zs[3] == 3 * n16 % 256 and zs[3] != 0 and (0 in hops or n16 >= 256)
    assert torch.equal(st.wave, plain.wave) and torch.equal(st.model, plain.model) and torch.equal(st.pkt[:, :256], plain.pkt[:, :256])
    for s in (0, 2, 3):
        want, lead = packet_reference(eng, win, fs, n, x[s], 0, g[s:s + 1])
        assert torch.equal(out[s], want), (fs, n, s)
        assert not out[s, :lead - (0 if fs == 16000 else lead // 4)].any()          # (other rates: up to the pre-ringing)
    want, lead = packet_reference(eng, win, fs, n, x[1, 3 * n:], zs[3], g[1:2])
    assert torch.equal(out[1, 3 * n:], want), (fs, n, "joined")
    if fs == 16000:             # bypass: the pre-fill and the z zeros of the join, then the input itself
        z = zs[3]
        assert not out[1, 3 * n:3 * n + lead + z].any()
        assert torch.equal(out[1, 3 * n + lead + z:], x[1, 3 * n:n * C - lead - z])
    assert torch.equal(out[3], outp[3]) and not torch.equal(out[0], outp[0])


def test_packet_calls_without_a_hop_launch_two_kernels_and_the_limit_can_be_switched_off(eng, win):
    """16 kHz / 160: launch records of a whole period with the limit on; then set_dry_gain(None) in the middle of a run
    returns to the plain output from the next block on (the blocks already in the outbound FIFO stay limited)."""
    n, N = 160, 3
    st = eng.new_packet_state(N, win, n, atten_lim_db=9)
    x1 = torch.randn(N, n, device="cuda") * 0.1
    seen = set()
    for _ in range(st.period):
        h = st.next_hops
        got = _launches(eng, lambda: eng.packet_stream_step(st, x1))
        if h == 0:
            assert got == {"k_packet_in": 1, "k_packet_out": 1}, got
        else:
            assert got.get("k_wave_synthesis_mix") == 1 and "k_wave_synthesis" not in got and sum(got.values()) == 5, got
        seen.add(h)
    assert seen == {0, 1}
    C, C1 = 40, 20
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(N, n * C, device="cuda", generator=gen) * 0.1
    sl, sp, sm = (eng.new_packet_state(N, win, n, atten_lim_db=9), eng.new_packet_state(N, win, n),
                  eng.new_packet_state(N, win, n, atten_lim_db=9))
    lim, _, hops = run_packets(eng, sl, x)
    pla, _, _ = run_packets(eng, sp, x)
    got, _, _ = run_packets(eng, sm, x, before={C1: lambda: sm.set_dry_gain(None)})
    assert sm.dry_gain is None
    cut = 256 - gcd(n, 256) + 256 * sum(hops[:C1])          # the pre-fill and the blocks emitted under the limit
    assert n * C1 < cut < n * C
    assert torch.equal(got[:, :cut], lim[:, :cut]) and torch.equal(got[:, cut:], pla[:, cut:])
    assert not torch.equal(lim[:, cut:], pla[:, cut:])


# ----------------------------------------------------------------------------------------------------------- 5. graphs
def test_captured_hop_step_follows_the_gains_on_the_device(eng, win):
    N, T = 16, 18
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, 256 * T, device="cuda", generator=gen) * 0.1
    sched = {0: 6, 6: [None, 0] * 8, 12: 15}                # the limits set before step t
    ref_st = eng.new_wave_state(N, win, atten_lim_db=3)
    ref = []
    for t in range(T):
        if t in sched:
            ref_st.set_atten_lim_db(sched[t])
        ref.append(eng.wave_stream_step(ref_st, x[:, 256 * t:256 * (t + 1)]).clone())
    xb, yb = torch.empty(N, 256, device="cuda"), torch.empty(N, 256, device="cuda")
    st, warm = eng.new_wave_state(N, win, atten_lim_db=3), eng.new_wave_state(N, win, atten_lim_db=3)
    eng.reserve(N, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        xb.copy_(x[:, :256])
        eng.wave_stream_step(warm, xb, out=yb)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            eng.wave_stream_step(st, xb, out=yb)
    eng.wave_stream_reset(st)
    torch.cuda.synchronize()
    ptr = st.dry_gain.data_ptr()
    for t in range(T):
        if t in sched:
            st.set_atten_lim_db(sched[t])
        xb.copy_(x[:, 256 * t:256 * (t + 1)])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yb, ref[t]), t
    assert st.dry_gain.data_ptr() == ptr                    # rewritten in place: the graph kept reading the same array
    assert torch.equal(st.model, ref_st.model) and torch.equal(st.wave, ref_st.wave)
    assert torch.equal(ref[8][1], x[1, 256 * 7:256 * 8]) and not torch.equal(ref[5][1], x[1, 256 * 4:256 * 5])


def test_captured_packet_period_follows_the_gains_on_the_device(eng, win):
    n, N = 160, 8
    st = eng.new_packet_state(N, win, n, atten_lim_db=6)
    P = st.period
    gen = torch.Generator(device="cuda").manual_seed(6)
    x = torch.randn(N, n * P * 3, device="cuda", generator=gen) * 0.1
    sched = {1: [0, 20] * 4, 2: None}                       # set before period r
    ref_st = eng.new_packet_state(N, win, n, atten_lim_db=6)
    ref = []
    for r in range(3):
        if r in sched:
            ref_st.set_atten_lim_db(sched[r])
        ref.append(run_packets(eng, ref_st, x[:, n * P * r:n * P * (r + 1)])[0])
    xb, yb = torch.empty(P, N, n, device="cuda"), torch.empty(P, N, n, device="cuda")
    warm = eng.new_packet_state(N, win, n, atten_lim_db=6)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        xb.copy_(x[:, :n * P].reshape(N, P, n).transpose(0, 1))
        for p in range(P):
            eng.packet_stream_step(warm, xb[p], out=yb[p])
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for p in range(P):
                eng.packet_stream_step(st, xb[p], out=yb[p])
    assert st.phase == 0
    eng.packet_stream_reset(st)
    torch.cuda.synchronize()
    for r in range(3):
        if r in sched:
            st.set_atten_lim_db(sched[r])
        xb.copy_(x[:, n * P * r:n * P * (r + 1)].reshape(N, P, n).transpose(0, 1))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yb.transpose(0, 1).reshape(N, P * n), ref[r]), r
    assert torch.equal(st.model, ref_st.model) and torch.equal(st.wave, ref_st.wave) and torch.equal(st.pkt, ref_st.pkt)


# ------------------------------------------------------------------------------------------ 6. launch counts and names
def test_a_limited_call_makes_the_launches_of_its_plain_form(eng, win):
    assert "k_wave_synthesis_mix" in eng.kernel_names() and "k_istft_mix" in eng.kernel_names()
    N = 8
    x = torch.randn(N, 256 * 12, device="cuda") * 0.1
    g = gains_for(N)

    def swapped(rec, a, b):
        rec = dict(rec)
        rec[b] = rec.pop(a)
        return rec

    plain = _launches(eng, lambda: eng.forward_wave(x, win))
    lim = _launches(eng, lambda: eng.forward_wave(x, win, dry_gain=g))
    assert plain["k_istft"] == 1 and "k_istft_mix" not in plain
    assert lim == swapped(plain, "k_istft", "k_istft_mix")
    lens = [256 * 12 - 10 * b for b in range(N)]
    plain = _launches(eng, lambda: eng.forward_wave_var(x, lens, win))
    lim = _launches(eng, lambda: eng.forward_wave_var(x, lens, win, dry_gain=g))
    assert lim == swapped(plain, "k_istft", "k_istft_mix")
    for nh in (1, 2, 5):
        sp, sl = eng.new_wave_state(N, win), eng.new_wave_state(N, win, atten_lim_db=6)
        plain = _launches(eng, lambda: eng.wave_stream_step(sp, x[:, :256 * nh]))
        lim = _launches(eng, lambda: eng.wave_stream_step(sl, x[:, :256 * nh]))
        assert plain["k_wave_synthesis"] == 1 and plain["k_wave_analysis"] == 1
        assert lim == swapped(plain, "k_wave_synthesis", "k_wave_synthesis_mix"), nh
        if nh == 1:
            assert sum(lim.values()) == 3
        plain = _launches(eng, lambda: eng.wave_stream_flush(sp, x[:, :17]))
        lim = _launches(eng, lambda: eng.wave_stream_flush(sl, x[:, :17]))
        assert lim == swapped(plain, "k_wave_synthesis", "k_wave_synthesis_mix") and sum(lim.values()) == 3
    rp, rl = eng.new_rate_state(N, win, 48000), eng.new_rate_state(N, win, 48000, atten_lim_db=6)
    plain = _launches(eng, lambda: eng.rate_stream_step(rp, x[:, :768]))
    lim = _launches(eng, lambda: eng.rate_stream_step(rl, x[:, :768]))
    assert lim == swapped(plain, "k_wave_synthesis", "k_wave_synthesis_mix")


# ------------------------------------------------------------------------------------------- 7. spectral equivalence
def test_time_domain_mix_equals_the_spectral_definition(eng, win):
    """beta X + (1 - beta) M X through the existing public calls; the two differ by the rounding of an STFT -> iSTFT round
    trip of the dry part.  Bound: the project's own, max|a - b| / max|b| <= 1e-4."""
    from gtcrn_micro_amd import stft, istft
    B, L = 8, 64000
    gen = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn(B, L, device="cuda", generator=gen) * 0.1
    beta = np.float32(G12)
    a = eng.forward_wave(x, win, dry_gain=float(beta))
    X = stft(x, win)
    b = istft(float(beta) * X + (1.0 - float(beta)) * eng.forward_spec(X), win)
    assert a.shape == b.shape
    err = float((a - b).abs().max() / b.abs().max())
    print(f"spectral equivalence: max|a-b| / max|b| = {err:.3e}")
    assert err <= 1e-4, err


# -------------------------------------------------------------------------------------------------- 8. non-regression
def test_plain_calls_after_limited_calls_are_unchanged(eng, win):
    """No sticky mode: the same handle, after limited calls of every form, gives a fresh handle's plain results."""
    from gtcrn_micro_amd import Engine
    N = 4
    gen = torch.Generator(device="cuda").manual_seed(8)
    x = torch.randn(N, 256 * 8 + 33, device="cuda", generator=gen) * 0.1
    eng.forward_wave(x, win, dry_gain=0.5)
    eng.wave_stream_step(eng.new_wave_state(N, win, atten_lim_db=6), x[:, :512])
    eng.rate_stream_step(eng.new_rate_state(N, win, 48000, atten_lim_db=6), x[:, :768])
    pk = eng.new_packet_state(N, win, 320, atten_lim_db=6)
    for c in range(4):
        eng.packet_stream_step(pk, x[:, 320 * c:320 * (c + 1)])
    fresh = Engine(load_params("dns3"), 0)

    def plain_everything(e, pkt):
        outs = [e.forward_wave(x, win), e.forward_wave_var(x, [x.shape[1] - 7 * b for b in range(N)], win,
                                                           out=torch.zeros(N, 2048, device="cuda"))]
        ws = e.new_wave_state(N, win)
        outs += [e.wave_stream_step(ws, x[:, :1024]), e.wave_stream_flush(ws, x[:, 1024:1100])]
        outs.append(e.rate_stream_step(e.new_rate_state(N, win, 48000), x[:, :1536]))
        outs += [e.packet_stream_step(pkt, x[:, 320 * c:320 * (c + 1)]) for c in range(5)]
        return outs
    pk.set_dry_gain(None)
    eng.packet_stream_reset(pk)
    # (the reused packet handle sits at phase 4 * 320 mod 256 = 0 again, as a new one does)
    assert pk.phase == 0
    for a, b in zip(plain_everything(eng, pk), plain_everything(fresh, fresh.new_packet_state(N, win, 320))):
        assert torch.equal(a, b)


def test_stream_wrapper_passes_the_limit_on(eng, win):
    from gtcrn_micro_amd.streaming.gtcrn_micro_stream import StreamGTCRNMicro
    stream = StreamGTCRNMicro().cuda().eval()
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(2, 256 * 4, device="cuda", generator=gen) * 0.1
    st = stream.init_wave_state(2, win, atten_lim_db=[6, 0])
    got = torch.cat([stream.step_wave(x[:, 256 * k:256 * (k + 1)], st) for k in range(4)], 1)
    e = stream.engine(x.device)
    assert torch.equal(got[:, 256:], limited_offline(e, win, x, st.dry_gain)[:, :768])
    assert stream.init_wave_state(2, win).dry_gain is None
    assert stream.init_wave_state(2, win, fs=48000, atten_lim_db=6).dry_gain.tolist() == [np.float32(G6)] * 2
    assert stream.init_wave_state(2, win, fs=16000, packet=160, atten_lim_db=6).dry_gain.tolist() == [np.float32(G6)] * 2
