"""The gain ramps (include/gtcrn_micro_hip.h, "gain ramps") on every live waveform path.  The checker
(tests/ramp_checker.py) is the contract in numpy float32, applied to the outputs of the PLAIN calls (which the other test
files pin) and the delayed inputs, as tests/test_gpu_dry_gain.py builds `mix_np`.  Every comparison is exact."""
import numpy as np
import pytest

from conftest import load_params
import meter_checker as MC
import ramp_checker as RK
import resample_checker as RC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
G6, G12 = F32(10.0 ** (-6 / 20)), F32(10.0 ** (-12 / 20))
GAINS = [F32(0.0), F32(1.0), G6, G12, F32(0.3718)]            # no limit, bypass, 6 dB, 12 dB, "a random value"
FFT_WAVES = 4                                                 # streams that share a synthesis workgroup


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


def i32(v):
    return torch.tensor(np.asarray(v, np.int32), dtype=torch.int32, device="cuda")


def noise(n, L, seed, amp=0.1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, L, device="cuda", generator=gen) * amp


def npf(t):
    return t.detach().cpu().numpy().astype(np.float32)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def put_gains(st, g):
    """Rewrites the state's gains in place (no snap: the ramp words stay)."""
    st.dry_gain.copy_(torch.from_numpy(np.asarray(g, np.float32)))


def delayed(x):
    """The dry samples under the blocks of a stream stepped from its reset: the input one hop late."""
    return np.concatenate([np.zeros_like(x[:, :256]), x[:, :-256]], 1)


def expect(w, x, gains, hops, first=0, p0=None):
    """The checker for N streams: w, x (N, 256 K) numpy; gains a list over calls of (N,) arrays."""
    ys, words = [], []
    for s in range(w.shape[0]):
        y, p = RK.ramped_stream(w[s], x[s], [g[s] for g in gains], hops, first,
                                None if p0 is None else p0[s])
        ys.append(y)
        words.append(p)
    return np.stack(ys), np.stack(words, 1)                   # (N, 256 K), (calls, N)


def schedule(N, calls, seed):
    """Per call: nhops from {1, 2, 3} and per-stream gains from GAINS; about a third of the streams keep theirs."""
    rng = np.random.default_rng(seed)
    hops = [int(h) for h in rng.integers(1, 4, calls)]
    g = np.array([GAINS[(s + seed) % len(GAINS)] for s in range(N)], np.float32)
    gains = []
    for c in range(calls):
        if c:
            move = rng.random(N) >= 0.35
            g = np.where(move, np.array(GAINS, np.float32)[rng.integers(0, len(GAINS), N)], g).astype(np.float32)
        gains.append(g)
    return hops, gains


# ------------------------------------------------------------------------------------------------------ 1. hop form
@pytest.mark.parametrize("N", [1, FFT_WAVES - 1, FFT_WAVES + 2])
@pytest.mark.parametrize("pcm", [False, True])
def test_hop_form_equals_the_checker(eng, win, N, pcm):
    """8 calls of 1..3 hops, the gains rewritten between calls.  The int16 form is the float form between the conversions:
    the ramp is mixed in float before the one rounding."""
    from gtcrn_micro_amd import pcm16_to_f32, f32_to_pcm16
    hops, gains = schedule(N, 8, 10 * N + pcm)
    K = sum(hops)
    if pcm:
        x16 = (noise(N, 256 * K, N, 3000.0)).round().clamp(-32768, 32767).to(torch.int16)
        xf = pcm16_to_f32(x16.contiguous())
    else:
        xf = noise(N, 256 * K, N)
    xin = x16 if pcm else xf
    st = eng.new_wave_state(N, win, atten_lim_db=None, ramp=True)
    plain, plain_in = eng.new_wave_state(N, win), eng.new_wave_state(N, win)
    assert st.gain_ramp.dtype == torch.float32 and tuple(st.gain_ramp.shape) == (N,)
    assert not st.gain_ramp.any() and not st.dry_gain.any()    # atten_lim_db=None: zeros, equal
    put_gains(st, gains[0])
    outs, ws, k = [], [], 0
    for h, g in zip(hops, gains):
        put_gains(st, g)
        sl = slice(256 * k, 256 * (k + h))
        outs.append(eng.wave_stream_step(st, xin[:, sl]))
        ws.append(eng.wave_stream_step(plain, xf[:, sl]))
        eng.wave_stream_step(plain_in, xin[:, sl])
        assert same(st.gain_ramp, torch.from_numpy(g)), k
        assert torch.equal(st.wave, plain_in.wave) and torch.equal(st.model, plain_in.model), k
        k += h
    want, _ = expect(npf(torch.cat(ws, 1)), delayed(npf(xf)), gains, hops)
    got = torch.cat(outs, 1)
    want = torch.from_numpy(want).cuda()
    assert torch.equal(got, f32_to_pcm16(want.contiguous())) if pcm else same(got, want)
    ramps = sum(1 for a, b in zip(gains, gains[1:]) if (a != b).any())
    assert ramps >= 3 and any((a == b).any() for a, b in zip(gains, gains[1:]))


def test_a_ramp_is_seen_and_is_not_a_step(eng, win):
    """0 -> 1 on one stream: the block between the enhanced and the dry signal is neither, starts 1/256 of the way and
    ends at the dry sample; the limited state steps."""
    N = 2
    x = noise(N, 256 * 4, 3)
    st, lim, plain = (eng.new_wave_state(N, win, atten_lim_db=None, ramp=True), eng.new_wave_state(N, win, atten_lim_db=None),
                      eng.new_wave_state(N, win))
    lim.set_atten_lim_db(None)
    for s in (st, lim, plain):
        eng.wave_stream_step(s, x[:, :512])
    st.set_atten_lim_db(0, 1, 2)
    lim.set_atten_lim_db(0, 1, 2)
    a, b, w = (eng.wave_stream_step(s, x[:, 512:768]) for s in (st, lim, plain))
    assert torch.equal(b[1], x[1, 256:512]) and torch.equal(a[0], w[0])
    assert not torch.equal(a[1], b[1]) and not torch.equal(a[1], w[1])
    assert same(a[1], torch.from_numpy(RK.mix(RK.R, npf(x[1, 256:512]), npf(w[1]))).cuda())
    assert float(a[1, 255]) == float(x[1, 511])
    a2, b2 = eng.wave_stream_step(st, x[:, 768:]), eng.wave_stream_step(lim, x[:, 768:])
    assert torch.equal(a2, b2)                                # behind the ramp: the limited stream


# -------------------------------------------------------------------------------------------------- 2. steady state
@pytest.mark.parametrize("meters", [False, True])
def test_steady_state_is_the_limited_call(eng, win, meters):
    N = 6
    x = noise(N, 256 * 7 + 100, 4)
    db = [None, 0, 6, 12, 8.59, 6]
    a = eng.new_wave_state(N, win, atten_lim_db=db, meters=meters, ramp=True)
    b = eng.new_wave_state(N, win, atten_lim_db=db, meters=meters)
    assert b.gain_ramp is None and same(a.gain_ramp, a.dry_gain)
    k = 0
    for h in (1, 2, 3, 1):
        assert same(eng.wave_stream_step(a, x[:, 256 * k:256 * (k + h)]), eng.wave_stream_step(b, x[:, 256 * k:256 * (k + h)]))
        k += h
    assert same(eng.wave_stream_flush(a, x[:, 256 * 7:]), eng.wave_stream_flush(b, x[:, 256 * 7:]))
    assert same(a.wave, b.wave) and same(a.model, b.model) and same(a.gain_ramp, a.dry_gain)
    if meters:
        assert same(a.meters, b.meters) and float(a.meters[0, 3]) == 8.0
    # two states on one engine do not leak: a step of the state without ramps leaves the words of the other alone
    a.set_atten_lim_db(3)
    before = a.gain_ramp.clone()
    eng.wave_stream_step(b, x[:, :256])
    assert same(a.gain_ramp, before) and not same(a.gain_ramp, a.dry_gain)
    a.set_atten_lim_db(20, snap=True)
    assert same(a.gain_ramp, a.dry_gain)


# ------------------------------------------------------------------------------------------------ 3. cut invariance
def test_the_cut_of_hops_into_calls_does_not_matter(eng, win):
    N = 5
    x = noise(N, 256 * 6, 5)
    outs = []
    for cut in ([4], [1, 1, 1, 1], [2, 2]):
        st = eng.new_wave_state(N, win, atten_lim_db=[None, 0, 6, 12, 6], ramp=True)
        eng.wave_stream_step(st, x[:, :512])
        st.set_atten_lim_db([0, None, 12, 12, 3])
        o, k = [], 2
        for h in cut:
            o.append(eng.wave_stream_step(st, x[:, 256 * k:256 * (k + h)]))
            k += h
        outs.append((torch.cat(o, 1), st.gain_ramp.clone(), st.wave.clone(), st.model.clone()))
    for other in outs[1:]:
        assert all(same(u, v) for u, v in zip(outs[0], other))
    assert same(outs[0][1], st.dry_gain)


# ---------------------------------------------------------------------------------------------------------- 4. join
def test_a_stream_that_joins_snaps(eng, win):
    """Slot 2's tenant is left at bypass; the slot is reset and its new stream asks for 12 dB: zeros, then 12 dB from the
    first sample.  A fresh state whose limit moves before its first step does the same."""
    N = 5
    x = noise(N, 256 * 6, 6)
    st = eng.new_wave_state(N, win, atten_lim_db=[6, 6, 0, 6, 6], ramp=True)
    plain = eng.new_wave_state(N, win)
    for s in (st, plain):
        eng.wave_stream_step(s, x[:, :768])
        eng.wave_stream_reset_slots(s, i32([2]))
    st.set_atten_lim_db(12, 2, 3)
    assert float(st.gain_ramp[2]) == 1.0 and float(st.dry_gain[2]) == float(G12)
    a, w = eng.wave_stream_step(st, x[:, 768:1024]), eng.wave_stream_step(plain, x[:, 768:1024])
    assert not a[2].any() and a[0].any() and same(st.gain_ramp, st.dry_gain)
    a, w = eng.wave_stream_step(st, x[:, 1024:1536]), eng.wave_stream_step(plain, x[:, 1024:1536])
    assert same(a[2], torch.from_numpy(RK.mix(G12, npf(x[2, 768:1280]), npf(w[2]))).cuda())
    fresh, plain = eng.new_wave_state(N, win, atten_lim_db=6, ramp=True), eng.new_wave_state(N, win)
    fresh.set_atten_lim_db(12)
    a, w = eng.wave_stream_step(fresh, x[:, :768]), eng.wave_stream_step(plain, x[:, :768])
    assert not a[:, :256].any() and same(fresh.gain_ramp, fresh.dry_gain)
    assert same(a[:, 256:], torch.from_numpy(RK.mix(G12, npf(x[:, :512]), npf(w[:, 256:]))).cuda())


# --------------------------------------------------------------------------------------------------------- 5. flush
@pytest.mark.parametrize("r", [0, 100])
def test_the_flush_block_ramps(eng, win, r):
    N = 3
    x = noise(N, 256 * 3 + r, 7 + r)
    st = eng.new_wave_state(N, win, atten_lim_db=[6, 12, None], ramp=True)
    plain = eng.new_wave_state(N, win)
    for s in (st, plain):
        eng.wave_stream_step(s, x[:, :768])
    g0 = npf(st.dry_gain)
    st.set_atten_lim_db([0, 12, 6])
    g1 = npf(st.dry_gain)
    a, w = eng.wave_stream_flush(st, x[:, 768:]), eng.wave_stream_flush(plain, x[:, 768:])
    dry = npf(x[:, 512:768])                                      # the ring's newest 256 samples
    want = np.stack([RK.mix(RK.ramp(g0[s], g1[s]), dry[s], npf(w[s])) for s in range(N)])
    assert same(a, torch.from_numpy(want).cuda())
    assert same(a[1], torch.from_numpy(RK.mix(G12, dry[1], npf(w[1]))).cuda())        # p == g: the limited flush
    assert same(st.gain_ramp, st.dry_gain) and same(st.wave, plain.wave) and same(st.model, plain.model)


def test_a_flush_without_a_block_stays_zero_and_sets_the_word(eng, win):
    N = 3
    x = noise(N, 256, 8) + 0.5
    st = eng.new_wave_state(N, win, atten_lim_db=6, ramp=True)
    assert not eng.wave_stream_step(st, x).any()
    st.set_atten_lim_db(0)
    assert not same(st.gain_ramp, st.dry_gain)
    assert not eng.wave_stream_flush(st, x[:, :0]).any()          # 256 samples in all: no block
    assert same(st.gain_ramp, st.dry_gain)
    st2 = eng.new_wave_state(N, win, atten_lim_db=6, ramp=True)
    st2.set_atten_lim_db(0)
    assert not eng.wave_stream_flush(st2, x[:, :200]).any()
    assert same(st2.gain_ramp, st2.dry_gain)


# --------------------------------------------------------------------------------------------------------- 6. slots
@pytest.mark.parametrize("pcm", [False, True])
def test_slots_ramp_the_named_and_leave_the_rest_alone(eng, win, pcm):
    """Seven resident streams; a call names slots 5, 1, 3 and, beyond the device count of 3, slot 6."""
    from gtcrn_micro_amd import pcm16_to_f32, f32_to_pcm16
    S = 7
    if pcm:
        x16 = noise(S, 256 * 4, 9, 3000.0).round().clamp(-32768, 32767).to(torch.int16)
        xf = pcm16_to_f32(x16.contiguous())
    else:
        xf = noise(S, 256 * 4, 9)
    xin = x16 if pcm else xf
    g0 = np.array([GAINS[s % 5] for s in range(S)], np.float32)
    g1 = np.array([GAINS[(s + 2) % 5] for s in range(S)], np.float32)
    st, plain = eng.new_wave_state(S, win, atten_lim_db=None, ramp=True), eng.new_wave_state(S, win)
    put_gains(st, g0)
    eng.wave_stream_step(st, xin[:, :512])
    eng.wave_stream_step(plain, xf[:, :512])
    put_gains(st, g1)
    table, cnt, named = i32([5, 1, 3, 6]), i32([3]), [5, 1, 3]
    rest = [s for s in range(S) if s not in named]
    before = [t.clone() for t in (st.gain_ramp, st.dry_gain, st.wave, st.model)]
    for k in (2, 3):
        rows = xin[[5, 1, 3, 6], 256 * k:256 * (k + 1)].contiguous()
        out = torch.full_like(rows, 77)
        eng.wave_stream_step_slots(st, table, rows, count=cnt, out=out)
        w = eng.wave_stream_step_slots(plain, table, xf[[5, 1, 3, 6], 256 * k:256 * (k + 1)].contiguous(), count=cnt)
        assert (out[3] == 77).all()                               # beyond the count: not written
        for i, s in enumerate(named):
            beta = RK.ramp(g0[s], g1[s]) if k == 2 else g1[s]
            want = torch.from_numpy(RK.mix(beta, npf(xf[s, 256 * (k - 1):256 * k]), npf(w[i]))).cuda()
            assert torch.equal(out[i], f32_to_pcm16(want.contiguous())) if pcm else same(out[i], want), (k, s)
        for t, b in zip((st.gain_ramp, st.dry_gain, st.wave, st.model), before):
            assert same(t[rest], b[rest]), k
        assert same(st.gain_ramp[named], st.dry_gain[named])
    assert (g0[rest] != g1[rest]).all() and any(g0[s] != g1[s] for s in named)


# -------------------------------------------------------------------------------------------------- 7. packet forms
def packet_out_of(eng, fs, n, C, b16):
    """The packet form's outbound stage applied to the 16 kHz blocks b16 (N, 256 H) of streams stepped from a reset at phase 0
    for C calls, as tests/test_gpu_dry_gain.py's packet_reference builds it: the pre-fill, then the resampler."""
    from gtcrn_micro_amd._lib import packet_stream_latency16
    n16 = n * 16000 // fs
    assert n16 * C % 256 == 0
    lat = packet_stream_latency16(fs, n)
    if fs == 16000:
        return torch.cat([b16.new_zeros(b16.shape[0], lat - 256), b16], 1)[:, :n * C]
    up, down, half, _ = RC.design(fs, 16000)
    upo, _, halfo, _ = RC.design(16000, fs)
    d_in, d_out = half // down, halfo // upo
    lead = lat - d_in - d_out
    assert lead >= 256
    B = torch.cat([b16.new_zeros(b16.shape[0], lead - 256), b16], 1)[:, :n16 * C]
    assert B.shape[1] == n16 * C
    rs = eng.resampler(16000, fs)
    return torch.stack([rs(torch.cat([B.new_zeros(d_out), B[s]]))[:n * C] for s in range(B.shape[0])])


def group_run(eng, win, fs, n, N, C, sched, x, feed=lambda t: t, **kw):
    """C packets through a ramped group and a plain one; sched {call: per-stream dB}.  Returns the outputs of both, the
    hand-offs a16 / b16 (ramped) / w16 (plain) and, per call with hops, the gains and the hop count."""
    st = eng.new_packet_state(N, win, n, fs, atten_lim_db=sched[0], ramp=True, **kw)
    plain = eng.new_packet_state(N, win, n, fs)
    assert same(st.gain_ramp, st.dry_gain)
    outs, outp, a16, b16, w16, gains, hops, seen = [], [], [], [], [], [], [], set()
    for c in range(C):
        if c and c in sched:
            st.set_atten_lim_db(sched[c])
        h, word = st.next_hops, st.gain_ramp.clone()
        seen.add(h)
        outs.append(eng.packet_stream_step(st, feed(x[:, n * c:n * (c + 1)].contiguous())))
        outp.append(eng.packet_stream_step(plain, x[:, n * c:n * (c + 1)].contiguous()))
        assert same(st.wave, plain.wave) and same(st.model, plain.model), c
        if h == 0:
            assert same(st.gain_ramp, word), c                    # no hop: the stream is not named, the word stays
            continue
        assert same(st.gain_ramp, st.dry_gain), c
        a16.append(eng.packet_stream_handoff(st, 0))
        b16.append(eng.packet_stream_handoff(st, 1))
        w16.append(eng.packet_stream_handoff(plain, 1))
        gains.append(npf(st.dry_gain))
        hops.append(h)
    cat = lambda v: torch.cat(v, 1)
    return cat(outs), cat(outp), cat(a16), cat(b16), cat(w16), gains, hops, seen


@pytest.mark.parametrize("fs,n,steps", [(16000, 160, {0, 1}), (16000, 320, {1, 2}), (48000, 480, {0, 1})])
def test_packet_group_hands_off_the_ramped_hop_stream(eng, win, fs, n, steps):
    N, C = 4, 16
    x = noise(N, n * C, fs + n) + 0.01
    sched = {0: [12, 0, 6, None], 3: [0, 0, None, 6], 4: [0, 12, None, 6], 9: [6, 6, 6, 6], 10: [None, 0, 6, 3]}
    out, outp, a16, b16, w16, gains, hops, seen = group_run(eng, win, fs, n, N, C, sched, x)
    assert seen == steps and sum(hops) == n * 16000 // fs * C // 256
    want, _ = expect(npf(w16), delayed(npf(a16)), gains, hops)
    assert same(b16, torch.from_numpy(want)), (fs, n)             # the 16 kHz hand-off is the ramped hop stream
    assert not same(b16, w16)
    assert same(outp, packet_out_of(eng, fs, n, C, w16))          # (the builder, on the plain form the other files pin)
    assert same(out, packet_out_of(eng, fs, n, C, b16)), (fs, n)  # the plain outbound stage applied to it


def test_g711_form_inherits_the_ramp(eng, win):
    """8 kHz / 160 mu-law: the codes are E_law of the float form's output, whose hand-off is the ramped hop stream."""
    from gtcrn_micro_amd import g711_to_f32, f32_to_g711
    fs, n, N, C = 8000, 160, 3, 8
    gen = torch.Generator(device="cuda").manual_seed(11)
    codes = torch.randint(0, 256, (N, n * C), device="cuda", generator=gen, dtype=torch.int32).to(torch.uint8)
    xf = g711_to_f32(codes.contiguous(), "ulaw")
    sched = {0: [12, 0, None], 2: [0, 6, 6], 5: [None, 6, 0]}
    outf, _, a16, b16, w16, gains, hops, _ = group_run(eng, win, fs, n, N, C, sched, xf)
    want, _ = expect(npf(w16), delayed(npf(a16)), gains, hops)
    assert same(b16, torch.from_numpy(want))
    outc, _, a16c, b16c, _, _, _, _ = group_run(eng, win, fs, n, N, C, sched, xf, g711="ulaw",
                                                feed=lambda t: f32_to_g711(t, "ulaw"))
    assert outc.dtype == torch.uint8 and same(a16c, a16) and same(b16c, b16)
    assert torch.equal(outc, f32_to_g711(outf.contiguous(), "ulaw"))


@pytest.mark.parametrize("fs,n", [(16000, 320), (48000, 480)])
def test_packet_slots_equal_ramped_one_stream_groups(eng, win, fs, n):
    """Five resident slots on a ragged schedule (so their phases differ), limits moving per slot; every slot is the ramped
    one-stream group fed the same packets, whose hand-off the test above holds against the checker."""
    S, T = 5, 10
    rng = np.random.default_rng(fs + n)
    db0 = [6, None, 0, 12, 6]
    st = eng.new_packet_slot_state(S, win, n, fs, atten_lim_db=db0, ramp=True)
    singles = [eng.new_packet_state(1, win, n, fs, atten_lim_db=db0[s], ramp=True) for s in range(S)]
    x = noise(S, n * T, fs + n + 1)
    fed = [0] * S
    moves = {2: {0: 0, 3: None}, 3: {1: 6}, 5: {0: 12, 2: 6, 4: None}, 7: {3: 0, 1: 0}}
    phases = set()
    for t in range(T):
        for s, db in moves.get(t, {}).items():
            st.set_atten_lim_db(db, s, s + 1)
            singles[s].set_atten_lim_db(db)
        act = [int(s) for s in rng.permutation(S) if rng.random() < 0.6] or [int(rng.integers(S))]
        if t == 0:
            act = [int(s) for s in rng.permutation(S)]
        xin = torch.stack([x[s, n * fed[s]:n * (fed[s] + 1)] for s in act])
        got = eng.packet_stream_step_slots(st, i32(act), xin)
        for i, s in enumerate(act):
            assert same(got[i:i + 1], eng.packet_stream_step(singles[s], xin[i:i + 1])), (t, s)
            fed[s] += 1
        assert same(st.gain_ramp, torch.cat([u.gain_ramp for u in singles])), t
        assert same(st.dry_gain, torch.cat([u.dry_gain for u in singles])), t
        phases.add(tuple(st.phase.tolist()))
    assert any(len(set(p)) > 1 for p in phases) and len(set(fed)) > 1


# ----------------------------------------------------------------------------------------------------- 8. rate form
def test_rate_form_ramps_at_16k(eng, win):
    fs, H, N = 48000, 768, 4
    x = noise(N, H * 7, 12)
    st = eng.new_rate_state(N, win, fs, atten_lim_db=[6, 0, None, 12], ramp=True)
    lim = eng.new_rate_state(N, win, fs, atten_lim_db=[6, 0, None, 12])
    plain = eng.new_rate_state(N, win, fs)
    sched = {1: [0, 0, 6, 12], 3: [None, 6, 6, 3]}
    a16, b16, w16, gains, hops, k = [], [], [], [], [1, 2, 1, 3], 0
    for c, nh in enumerate(hops):
        if c in sched:
            st.set_atten_lim_db(sched[c])
            lim.set_atten_lim_db(sched[c])
        got = eng.rate_stream_step(st, x[:, H * k:H * (k + nh)])
        a16.append(eng.rate_stream_handoff(st, nh, 0))
        b16.append(eng.rate_stream_handoff(st, nh, 1))
        ref = eng.rate_stream_step(lim, x[:, H * k:H * (k + nh)])
        eng.rate_stream_step(plain, x[:, H * k:H * (k + nh)])
        w16.append(eng.rate_stream_handoff(plain, nh, 1))
        assert same(st.wave, plain.wave) and same(st.model, plain.model) and same(st.gain_ramp, st.dry_gain), c
        assert same(got[3], ref[3]) == (c != 3)                   # stream 3 moves once, before call 3
        gains.append(npf(st.dry_gain))
        k += nh
    a16, b16, w16 = (torch.cat(v, 1) for v in (a16, b16, w16))
    want, _ = expect(npf(w16), delayed(npf(a16)), gains, hops)
    assert same(b16, torch.from_numpy(want)) and not same(b16, w16)


# -------------------------------------------------------------------------------------------------------- 9. meters
def test_meters_take_the_ramped_samples(eng, win):
    N = 5
    hops, gains = schedule(N, 5, 13)
    K = sum(hops)
    x = noise(N, 256 * K, 13)
    st = eng.new_wave_state(N, win, atten_lim_db=None, meters=True, ramp=True)
    plain = eng.new_wave_state(N, win)
    outs, ws, k = [], [], 0
    for h, g in zip(hops, gains):
        put_gains(st, g)
        outs.append(eng.wave_stream_step(st, x[:, 256 * k:256 * (k + h)]))
        ws.append(eng.wave_stream_step(plain, x[:, 256 * k:256 * (k + h)]))
        k += h
    dry = delayed(npf(x))
    want, _ = expect(npf(torch.cat(ws, 1)), dry, gains, hops)
    assert same(torch.cat(outs, 1), torch.from_numpy(want))
    rec = npf(st.meters)
    for s in range(N):
        yb, xb = want[s].reshape(-1, 256), dry[s].reshape(-1, 256)
        MC.check(rec[s], yb, xb, what=s)
        assert MC.same_bits(rec[s], MC.emulate(yb, xb)), s
    assert any((a != b).any() for a, b in zip(gains, gains[1:]))


# ------------------------------------------------------------------------------------------------------- 10. capture
def test_a_captured_step_follows_the_gains_between_replays(eng, win):
    N = 6
    x = noise(N, 256 * 7, 14)
    sched = {2: 6, 3: [None, 0, 6, 12, 3, 0], 4: 0, 5: [6, 6, None, None, 12, 0], 6: 20}
    ref_st = eng.new_wave_state(N, win, atten_lim_db=3, ramp=True)
    ref = []
    for t in range(7):
        if t in sched:
            ref_st.set_atten_lim_db(sched[t])
        ref.append(eng.wave_stream_step(ref_st, x[:, 256 * t:256 * (t + 1)]).clone())
    xb, yb = torch.empty(N, 256, device="cuda"), torch.empty(N, 256, device="cuda")
    st, warm = (eng.new_wave_state(N, win, atten_lim_db=3, ramp=True) for _ in range(2))
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
    for t in range(2):                                            # the eager steps in front of the five replays
        xb.copy_(x[:, 256 * t:256 * (t + 1)])
        assert same(eng.wave_stream_step(st, xb), ref[t])
    for t in range(2, 7):
        st.set_atten_lim_db(sched[t])
        xb.copy_(x[:, 256 * t:256 * (t + 1)])
        g.replay()
        torch.cuda.synchronize()
        assert same(yb, ref[t]), t
    assert same(st.gain_ramp, ref_st.gain_ramp) and same(st.model, ref_st.model) and same(st.wave, ref_st.wave)


# ----------------------------------------------------------------------------------------------------- 11. isolation
def test_a_nan_in_one_stream_leaves_the_other_streams_ramp_alone(eng, win):
    """Streams 0 and 1 share a workgroup; stream 0's input turns NaN in the hop during which stream 1 ramps."""
    N = 3
    x = noise(N, 256 * 5, 15)
    xb = x.clone()
    xb[0, 256 * 2 + 17] = float("nan")
    runs = []
    for inp in (x, xb):
        st = eng.new_wave_state(N, win, atten_lim_db=[6, 12, 0], ramp=True)
        o = [eng.wave_stream_step(st, inp[:, :512])]
        st.set_atten_lim_db([0, 0, 6])
        o.append(eng.wave_stream_step(st, inp[:, 512:768]))
        st.set_atten_lim_db([6, None, 6])
        o.append(eng.wave_stream_step(st, inp[:, 768:]))
        runs.append((torch.cat(o, 1), st.gain_ramp.clone(), st.wave.clone(), st.model.clone()))
    (a, ra, wa, ma), (b, rb, wb, mb) = runs
    assert torch.isnan(b[0]).any() and not torch.isnan(a).any()
    for v in (1, 2):
        assert same(a[v], b[v]) and same(wa[v], wb[v]) and same(ma[v], mb[v]), v
    assert same(ra, rb)
