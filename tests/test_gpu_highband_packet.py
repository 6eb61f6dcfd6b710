"""The high band on the packet forms on the GPU (gtcrn_packet_stream_step_hb / _step_slots_hb; contract:
include/gtcrn_micro_hip.h, "high band on the packet forms"): the exact bypass (also for a stream that joins mid-period),
gamma = 0 against the plain and the limited call, 48 kHz / 768 against the rate form's high band, the contract against
tests/highband_packet_checker.py, a tone above the band, int16 against float, the slot form against one-stream groups, a
captured slot call, the launch records, the meters and the argument errors.  Three streams in a group, or five resident slots
of which three step per call; 16 - 24 calls per test: two periods and past the latency."""
import ctypes
from math import gcd

import numpy as np
import pytest

from conftest import load_params
import highband_packet_checker as PC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 3                                   # streams of a group
S, M = 5, 3                             # resident slots, max_active
CASES = [(48000, 480), (48000, 960), (32000, 320), (24000, 240)]
LAT = {(48000, 480): 1632, (48000, 960): 1536, (48000, 768): 960, (32000, 320): 1088, (24000, 240): 816}


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


def i32(ids):
    return torch.tensor(list(ids), dtype=torch.int32, device="cuda")


def noise(rows, cols, seed, scale=0.1, pcm=False):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(rows, cols, device="cuda", generator=gen) * scale
    if pcm:
        x = (x * 32768).round().clamp(-32768, 32767).to(torch.int16)
    return x


def calls_for(fs, n):
    """Two periods at least, past the latency, 16 - 24 calls."""
    n16 = n * 16000 // fs
    return max(16, 2 * (256 // gcd(n16, 256)))


def run(eng, st, x, k0=0, k1=None, taps=None):
    """Packets k0 .. k1 - 1 of x (rows, n K) through the group state; taps: a list that receives (A hops, W hops) per call."""
    n = st.packet
    k1 = x.shape[1] // n if k1 is None else k1
    outs = []
    for k in range(k0, k1):
        outs.append(eng.packet_stream_step(st, x[:, n * k:n * (k + 1)]).clone())
        if taps is not None:
            taps.append((eng.packet_stream_handoff(st, 0), eng.packet_stream_handoff(st, 1)))
    return torch.cat(outs, 1)


def states(st):
    return [st.model, st.wave, st.pkt] + ([st.hb] if st.hb is not None else [])


def delayed(x, lat):
    return torch.cat([torch.zeros(x.shape[0], lat, device="cuda", dtype=x.dtype), x], 1)[:, :x.shape[1]]


# ------------------------------------------------------------------------------------------------ 1. the exact bypass
@pytest.mark.parametrize("fs,n", CASES)
@pytest.mark.parametrize("pcm", [False, True])
def test_bypass_is_exact_also_for_a_stream_that_joins_mid_period(eng, win, fs, n, pcm):
    """atten_lim_db = 0 and highband = 1: out == zeros(LAT) ++ x, bit for bit, at the caller's packet size (n < LAT: the
    delay line shifts in every call; 48 kHz / 960 steps h = 1 and h = 2).  Stream 1 is reset at a non-zero group phase and
    bypasses its new clip at the same LAT."""
    K = calls_for(fs, n)
    x = noise(N, n * K, fs + n, 0.3, pcm)
    st = eng.new_packet_state(N, win, n, fs, atten_lim_db=0, highband=1.0)
    lat = st.hb_latency
    assert lat == LAT[(fs, n)] and lat > n and (n != 480 or st.hb.shape[1] * 4 == 8448)
    hops, r, first = [], None, []
    for k in range(K):
        if r is None and k >= 3 and st.phase != 0:
            r = k
            eng.packet_stream_reset(st, 1, 2)
            assert not st.hb[1].any() and not st.pkt[1].any() and st.hb[0].any() and st.hb[2].any()
        hops.append(st.next_hops)
        first.append(eng.packet_stream_step(st, x[:, n * k:n * (k + 1)]).clone())
    out = torch.cat(first, 1)
    assert r is not None and out.dtype == x.dtype
    assert set(hops) == ({1, 2} if n == 960 else {0, 1})
    want = delayed(x, lat)
    assert torch.equal(out[0], want[0]) and torch.equal(out[2], want[2]), int((out != want).sum())
    assert torch.equal(out[1, :n * r], want[1, :n * r])
    assert torch.equal(out[1:2, n * r:], delayed(x[1:2, n * r:], lat)), (fs, n, r)
    assert out[0, lat:].any() and out[1, n * r + lat:].any()


# ------------------------------------------------------------------------------------------------ 2. gamma = 0
@pytest.mark.parametrize("fs,n", CASES)
@pytest.mark.parametrize("lim", [None, 12.0])
@pytest.mark.parametrize("pcm", [False, True])
def test_gain_zero_equals_the_plain_and_the_limited_call(eng, win, fs, n, lim, pcm):
    K = calls_for(fs, n)
    x = noise(N, n * K, fs + n + 2, 0.1, pcm)
    ref = eng.new_packet_state(N, win, n, fs, atten_lim_db=lim)
    st = eng.new_packet_state(N, win, n, fs, atten_lim_db=lim, highband=0.0)
    want, got = run(eng, ref, x), run(eng, st, x)
    assert torch.equal(got, want) and got.any()                    # (==: a zero may differ in sign)
    for a, b in zip(states(ref), states(st)):
        assert torch.equal(a, b)
    assert ref.phase == st.phase and st.hb.any()


# ------------------------------------------------------------------------------------------------ 3. 48 kHz / 768 is the rate form
@pytest.mark.parametrize("lim", [None, 12.0])
@pytest.mark.parametrize("pcm", [False, True])
def test_768_sample_packets_equal_the_rate_form_call_by_call(eng, win, lim, pcm):
    fs, n, K = 48000, 768, 8
    x = noise(N, n * K, 768, 0.1, pcm)
    rt = eng.new_rate_state(N, win, fs, atten_lim_db=lim, highband=0.5)
    st = eng.new_packet_state(N, win, n, fs, atten_lim_db=lim, highband=0.5)
    assert st.phase == 0 and st.hb_latency == rt.latency == 960 and st.hb.shape == rt.hb.shape
    for k in range(K):
        a = eng.rate_stream_step(rt, x[:, n * k:n * (k + 1)])
        b = eng.packet_stream_step(st, x[:, n * k:n * (k + 1)])
        assert torch.equal(a, b), k
        assert torch.equal(st.hb, rt.hb), k
    assert b.any() and torch.equal(st.model, rt.model) and torch.equal(st.wave, rt.wave)


# ------------------------------------------------------------------------------------------------ 4. the contract
@pytest.mark.parametrize("fs,n,lim", [(48000, 480, None), (48000, 480, 12.0), (48000, 960, None), (32000, 320, None),
                                      (24000, 240, 12.0)])
def test_contract_against_the_checker(eng, win, fs, n, lim):
    """Per-stream gains (0.25, 0.5, 1.0) on a group at phase 0: the hand-off hops of the calls concatenate to A and to the
    wave step's output W, and P = zeros(256 - g) ++ W.  Tolerance: the checker's own bound (the fp32 dot-product bound on the
    outbound stage plus two fp32 roundings of the mix)."""
    from gtcrn_micro_amd._lib import resample_taps
    up, down, h = resample_taps(16000, fs)
    gains = (0.25, 0.5, 1.0)
    K = calls_for(fs, n)
    n16 = n * 16000 // fs
    g = gcd(n16, 256)
    x = noise(N, n * K, fs + n + 3)
    st = eng.new_packet_state(N, win, n, fs, atten_lim_db=lim, highband=gains)
    taps = []
    out = run(eng, st, x, taps=taps).cpu().numpy().astype(np.float64)
    T = n16 * K
    A = torch.cat([t[0] for t in taps], 1).cpu().numpy()
    W = torch.cat([t[1] for t in taps], 1).cpu().numpy()
    assert A.shape[1] == 256 * (T // 256) and T - A.shape[1] == st.phase
    # A is needed up to T - L16 and W up to T - (256 - g): both are inside the hops that were handed over
    A = np.concatenate([A, np.zeros((N, T - A.shape[1]), np.float32)], 1)
    P = np.concatenate([np.zeros((N, 256 - g), np.float32), W], 1)[:, :T]
    assert P.shape[1] == T
    xs = x.cpu().numpy()
    worst = 0.0
    for s in range(N):
        r = PC.live(A[s], P[s], xs[s], gains[s], 512 - g, 32, up, down, h)
        assert r["lat"] == LAT[(fs, n)]
        err = np.abs(out[s] - r["out"])
        nz = r["bound"] > 0
        worst = max(worst, float((err[nz] / r["bound"][nz]).max()))
        assert (err <= r["bound"]).all(), (fs, n, lim, s, float((err - r["bound"]).max()))
        assert np.abs(r["dry"]).max() > 0.01 and np.abs(r["v"]).max() > 1e-3      # both terms are in play
    print(f"fs {fs} n {n} limit {lim}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 5. a tone above the band
def _tone_amplitude(y, f, fs, start):
    seg = y[start:].astype(np.float64)
    t = np.arange(seg.size)
    wnd = np.hanning(seg.size)
    return 2 * abs(np.sum(seg * wnd * np.exp(-2j * np.pi * f * t / fs))) / wnd.sum()


def test_a_tone_above_the_band_survives(eng, win):
    """A 12 kHz tone of amplitude 0.25 at 48 kHz / 480, gamma = 0.5: the output's projection on the tone has amplitude 0.125
    (within 1e-4, the margin of the float64 statement in tests/test_highband_packet_host.py), where the plain call leaves
    less than 1e-10 of it (both stages are >= 96 dB down at the tone)."""
    fs, n, f, K = 48000, 480, 12000.0, 24
    t = np.arange(n * K)
    x = cu(np.tile((0.25 * np.sin(2 * np.pi * f * t / fs + 0.3)).astype(np.float32), (N, 1)))
    hb = run(eng, eng.new_packet_state(N, win, n, fs, highband=0.5), x).cpu().numpy()
    plain = run(eng, eng.new_packet_state(N, win, n, fs), x).cpu().numpy()
    start = LAT[(fs, n)] + 400
    for s in range(N):
        got, base = _tone_amplitude(hb[s], f, fs, start), _tone_amplitude(plain[s], f, fs, start)
        print(f"stream {s}: tone amplitude {got:.7f} with the high band, {base:.2e} without")
        assert abs(got - 0.125) <= 1e-4, (s, got)
        assert base < 1e-10, (s, base)


# ------------------------------------------------------------------------------------------------ 6. int16 between the conversions
@pytest.mark.parametrize("fs,n", [(48000, 480), (24000, 240)])
def test_pcm16_equals_the_float_form_between_the_two_conversions(eng, win, fs, n):
    from gtcrn_micro_amd import f32_to_pcm16, pcm16_to_f32
    K = calls_for(fs, n)
    xi = noise(N, n * K, fs + 6, 0.2, True)
    gains = (1.0, 0.5, 0.25)
    si = eng.new_packet_state(N, win, n, fs, atten_lim_db=6.0, highband=gains)
    sf = eng.new_packet_state(N, win, n, fs, atten_lim_db=6.0, highband=gains)
    got = run(eng, si, xi)
    want = f32_to_pcm16(run(eng, sf, pcm16_to_f32(xi)))
    assert got.dtype == torch.int16 and torch.equal(got, want) and got.any()
    for a, b in zip(states(si), states(sf)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. slots
SLOT_GAINS = (0.25, 0.5, 1.0, 0.75, 0.3)


def slot_schedule(ticks):
    """Per tick at most M of the slots 0..3 (slot 4 is never named): slot 0 at every tick, slot 1 loses every third packet,
    slot 2 is in from tick 2, slot 3 steps ticks 0..2, leaves, and JOINS again at tick 7 through the reset kernel."""
    sched = []
    for t in range(ticks):
        ids = [0]
        if t % 3 != 1:
            ids.append(1)
        if t >= 2 and len(ids) < M and (t % 2 or t >= 7):
            ids.append(2)
        if (t <= 2 or t >= 7) and len(ids) < M:
            ids.append(3)
        sched.append(ids[::-1] if t % 2 else ids)
    return sched


def truth(eng, win, fs, n, packets, gain):
    """A one-stream group created at phase 0, the same gain, fed `packets` (k, n): (outputs, state)."""
    st = eng.new_packet_state(1, win, n, fs, atten_lim_db=9.0, highband=gain)
    assert st.phase == 0
    outs = [eng.packet_stream_step(st, packets[k:k + 1]).clone() for k in range(packets.shape[0])]
    return torch.cat(outs, 1)[0], st


@pytest.mark.parametrize("fs,n,pcm", [(48000, 480, False), (48000, 960, True), (24000, 240, False)])
def test_each_slot_is_a_one_stream_group_at_phase_zero(eng, win, fs, n, pcm):
    """Slot 1 skips calls (lost packets), slot 3 leaves and joins at a later tick through the reset kernel, slot 4 is never
    named: every slot equals its one-stream truth bit for bit, outputs and all four states and the phase word, and the slot
    that is not named keeps its bytes, in d_hbstate too."""
    ticks = calls_for(fs, n) + 4
    sched = slot_schedule(ticks)
    assert all(len(t) <= M and 4 not in t for t in sched) and any(len(t) == M for t in sched)
    x = noise(S, n * ticks, fs + n + 7, 0.1, pcm)
    st = eng.new_packet_slot_state(S, win, n, fs, max_active=M, atten_lim_db=9.0, highband=SLOT_GAINS)
    assert st.hb.shape == (S, LAT[(fs, n)] + 512 - gcd(n * 16000 // fs, 256)) and not st.hb.any()
    for t_ in (st.model, st.wave, st.pkt, st.hb):
        t_[4].fill_(-3.25)                                                     # a slot nobody names: sentinel bytes
    st.phase[4] = 128
    keep = [t_[4].clone() for t_ in (st.model, st.wave, st.pkt, st.hb)]
    seen, first = [0] * S, [0] * S
    blocks = [[] for _ in range(S)]
    xin = torch.zeros((M, n), device="cuda", dtype=x.dtype)
    out = torch.empty((M, n), device="cuda", dtype=x.dtype)
    fill = 77 if pcm else -7.0
    for t, ids in enumerate(sched):
        if t == 7:
            assert st.hb[3].any() and int(st.phase[3]) == (3 * (n * 16000 // fs)) % 256
            before = [u.clone() for u in (st.model, st.wave, st.pkt, st.hb, st.phase)]
            eng.packet_stream_reset_slots(st, i32([3, 0, 1]), count=i32([1]))       # (count 1: slots 0 and 1 are not reset)
            assert not st.hb[3].any() and not st.pkt[3].any() and int(st.phase[3]) == 0
            for u, b in zip((st.model, st.wave, st.pkt, st.hb, st.phase), before):
                others = [s for s in range(S) if s != 3]
                assert torch.equal(u[others].view(torch.int32), b[others].view(torch.int32))
            first[3], blocks[3] = seen[3], []
        table = i32(ids + [s for s in range(S) if s not in ids][:M - len(ids)])
        xin.zero_()
        for i, s in enumerate(ids):
            xin[i] = x[s, n * seen[s]:n * (seen[s] + 1)]
        out.fill_(fill)
        eng.packet_stream_step_slots(st, table, xin, count=i32([len(ids)]), out=out)
        assert torch.equal(out[len(ids):], torch.full_like(out[len(ids):], fill)), "rows at or beyond count were written"
        for i, s in enumerate(ids):
            blocks[s].append(out[i].clone())
            seen[s] += 1
    for s in range(4):
        pk = x[s, n * first[s]:n * seen[s]].reshape(seen[s] - first[s], n)
        want, ts = truth(eng, win, fs, n, pk, SLOT_GAINS[s])
        got = torch.cat(blocks[s])
        assert torch.equal(got, want) and got.any(), (fs, n, s)
        for a, b in zip(states(st), states(ts)):
            assert torch.equal(a[s:s + 1], b), (fs, n, s)
        assert int(st.phase[s]) == ts.phase, (fs, n, s)
    assert seen[1] < seen[0] and first[3] == 3 and seen[3] - first[3] > LAT[(fs, n)] // n
    for u, b in zip((st.model, st.wave, st.pkt, st.hb), keep):
        assert torch.equal(u[4].view(torch.int32), b.view(torch.int32))
    assert int(st.phase[4]) == 128


def test_one_captured_slot_call_follows_gains_and_active_sets(eng, win):
    """ONE capture of ONE call (48 kHz / 480: a period is 8 ticks), replayed for 18 ticks with the table, the count, the
    packets and the high-band gains rewritten between replays, equals the eager run."""
    fs, n, ticks = 48000, 480, 18
    x = noise(S, n * ticks, 4242)
    rng = np.random.default_rng(11)
    plan = [(rng.permutation(S)[:M], c) for c in [3, 0, 2, 3, 1, 3, 2, 0, 3, 3, 1, 2, 3, 3, 2, 1, 3, 3]]
    assert len(plan) == ticks > 2 * (256 // gcd(160, 256))
    seen, inputs = [0] * S, []
    for perm, c in plan:
        xin = torch.zeros((M, n), device="cuda")
        for i in range(c):
            s = int(perm[i])
            xin[i] = x[s, n * seen[s]:n * (seen[s] + 1)]
            seen[s] += 1
        inputs.append(xin)
    gains = lambda k: SLOT_GAINS if k < 9 else (1.0, 0.0, 0.5, 0.25, 0.75)          # noqa: E731

    se = eng.new_packet_slot_state(S, win, n, fs, max_active=M, highband=SLOT_GAINS)
    eager = []
    for k, ((p, c), xin) in enumerate(zip(plan, inputs)):
        se.set_highband_gain(gains(k))
        eager.append(eng.packet_stream_step_slots(se, i32(p), xin, count=i32([c])).clone()[:c])
    assert len(set(se.phase.tolist())) > 2 and se.hb.any()
    sg = eng.new_packet_slot_state(S, win, n, fs, max_active=M, highband=SLOT_GAINS)
    slots, count = i32(plan[0][0]), i32([0])
    xin, out = torch.zeros((M, n), device="cuda"), torch.zeros((M, n), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.packet_stream_step_slots(sg, slots, xin, count=count, out=out)    # warm-up with count 0: nothing steps
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.packet_stream_step_slots(sg, slots, xin, count=count, out=out)
    for k, ((p, c), xk) in enumerate(zip(plan, inputs)):
        slots.copy_(i32(p))
        count.fill_(c)
        xin.copy_(xk)
        sg.set_highband_gain(gains(k))
        graph.replay()
        assert torch.equal(out[:c], eager[k]), k
    for a, b in zip(states(sg) + [sg.phase], states(se) + [se.phase]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 8. launch records, meters
def _launches(eng, fn):
    eng.timing_enable(True)
    fn()
    torch.cuda.synchronize()
    t = {k: v[1] for k, v in eng.timing_read().items()}
    eng.timing_enable(False)
    return t


@pytest.mark.parametrize("fs,n", [(48000, 480), (48000, 960)])
def test_launch_records_equal_the_plain_forms(eng, win, fs, n):
    """A high-band call makes the launches of its plain form one for one (the outbound kernel's row counts the high-band
    kernel), the two launches of an h = 0 call included; the slot call likewise."""
    plain, st = eng.new_packet_state(N, win, n, fs), eng.new_packet_state(N, win, n, fs, highband=0.5)
    x = noise(N, n, 1)
    y = torch.empty_like(x)
    hops = set()
    for _ in range(st.period):
        assert plain.next_hops == st.next_hops
        hops.add(st.next_hops)
        a = _launches(eng, lambda: eng.packet_stream_step(plain, x, out=y))
        b = _launches(eng, lambda: eng.packet_stream_step(st, x, out=y))
        assert a == b and a["k_packet_in"] == 1 and a["k_packet_out"] == 1, (a, b)
        if st.last_hops == 0:
            assert a == {"k_packet_in": 1, "k_packet_out": 1}
    assert hops == ({1, 2} if n == 960 else {0, 1})
    sp = eng.new_packet_slot_state(S, win, n, fs, max_active=M)
    sh = eng.new_packet_slot_state(S, win, n, fs, max_active=M, highband=0.5)
    for k in range(4):
        ids, c = i32([(k + j) % S for j in range(M)]), i32([k % (M + 1)])
        a = _launches(eng, lambda: eng.packet_stream_step_slots(sp, ids, x, count=c, out=y))
        b = _launches(eng, lambda: eng.packet_stream_step_slots(sh, ids, x, count=c, out=y))
        assert a == b and a["k_packet_plan"] == 1 and a["k_packet_in_slots"] == 1 and a["k_packet_out_slots"] == 1, (a, b)


def test_meters_equal_the_plain_forms(eng, win):
    """The wave step is called exactly as it is: the level records of a metered high-band state are those of the plain one."""
    fs, n, K = 48000, 480, 16
    x = noise(N, n * K, 31)
    bits = lambda t: t.view(torch.int32)                                           # noqa: E731
    a = eng.new_packet_state(N, win, n, fs, atten_lim_db=6.0, meters=True)
    b = eng.new_packet_state(N, win, n, fs, atten_lim_db=6.0, meters=True, highband=(0.25, 0.5, 1.0))
    for k in range(K):
        eng.packet_stream_step(a, x[:, n * k:n * (k + 1)])
        eng.packet_stream_step(b, x[:, n * k:n * (k + 1)])
        assert torch.equal(bits(a.meters), bits(b.meters)), k
    assert a.meters.any() and (a.meters[:, 3] == (160 * K) // 256).all()
    sa = eng.new_packet_slot_state(S, win, n, fs, max_active=M, meters=True)
    sb = eng.new_packet_slot_state(S, win, n, fs, max_active=M, meters=True, highband=SLOT_GAINS)
    for k in range(K):
        ids = i32([(k + j) % S for j in range(M)])
        eng.packet_stream_step_slots(sa, ids, x[:, n * k:n * (k + 1)])
        eng.packet_stream_step_slots(sb, ids, x[:, n * k:n * (k + 1)])
    assert sa.meters.any() and torch.equal(bits(sa.meters), bits(sb.meters))


# ------------------------------------------------------------------------------------------------ 9. the wrapper, errors
def test_stream_wrapper_takes_the_high_band(eng, win):
    from gtcrn_micro_amd._lib import PacketSlotState, PacketStreamState
    from gtcrn_micro_amd.streaming.gtcrn_micro_stream import StreamGTCRNMicro
    stream = StreamGTCRNMicro().cuda().eval()
    fs, n, K = 48000, 480, 16
    x = noise(2, n * K, 8)
    st = stream.init_wave_state(2, win, fs=fs, packet=n, highband=(0.5, 1.0))
    assert isinstance(st, PacketStreamState) and st.hb is not None and st.hb_latency == 1632
    got = torch.cat([stream.step_wave(x[:, n * k:n * (k + 1)], st) for k in range(K)], 1)
    e = stream.engine(x.device)
    want = run(e, e.new_packet_state(2, win, n, fs, highband=(0.5, 1.0)), x)
    assert torch.equal(got, want) and got.any()
    plain = stream.init_wave_state(2, win, fs=fs, packet=n)
    assert plain.hb is None and plain.hb_gain is None
    assert not torch.equal(run(e, plain, x), want)
    rs = stream.init_wave_state(S, win, fs=fs, packet=n, resident=True, max_active=M, highband=0.5)
    assert isinstance(rs, PacketSlotState) and rs.hb is not None and rs.hb_gain.shape == (S,)
    stream.step_wave(x[:, :n], rs, slots=i32([4, 2]))
    assert rs.hb[4].any() and rs.hb[2].any() and not rs.hb[0].any()
    stream.init_wave_state(S, win, state=rs, slots=i32([4]))
    assert not rs.hb[4].any() and rs.hb[2].any()


def test_errors_are_raised_before_any_launch(eng, win):
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import lib
    fs, n = 48000, 480
    for kw in (dict(fs=16000, packet=160), dict(fs=8000, packet=160), dict(fs=44100, packet=441), dict(fs=22050, packet=441)):
        with pytest.raises(GtcrnError):
            eng.new_packet_state(N, win, kw["packet"], kw["fs"], highband=0.5)
        with pytest.raises(GtcrnError):
            eng.new_packet_slot_state(S, win, kw["packet"], kw["fs"], highband=0.5)
    with pytest.raises(GtcrnError):
        eng.new_packet_state(N, win, n, fs, highband=1.5)
    with pytest.raises(GtcrnError):
        eng.new_packet_state(N, win, 160, 8000, g711="ulaw", highband=0.5)
    with pytest.raises(GtcrnError):
        eng.new_packet_slot_state(S, win, n, fs, g711="alaw", highband=0.5)
    with pytest.raises(GtcrnError):
        eng.new_packet_state(N, win, n, fs).set_highband_gain(0.5)
    st = eng.new_packet_state(N, win, n, fs, highband=0.5)
    x = noise(N, n, 2)
    eng.packet_stream_step(st, x)
    b0 = [t.clone() for t in states(st)]
    ph = st.phase
    L, sp = lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.full((N, n), 7.0, device="cuda")
    big = torch.zeros(N, 2 * n, device="cuda")

    def raw(xp=None, xs=n, op=None, os_=n, hb=0, gain=0):
        return L.gtcrn_packet_stream_step_hb(st._h, st.model.data_ptr(), st.wave.data_ptr(), st.pkt.data_ptr(),
                                             x.data_ptr() if xp is None else xp, xs, out.data_ptr() if op is None else op, os_,
                                             N, st.window.data_ptr(), st.hb.data_ptr() if hb == 0 else hb,
                                             st.hb_gain.data_ptr() if gain == 0 else gain, sp)

    def nothing_ran(fn):
        got = _launches(eng, fn)
        assert not any(got.values()), got
        assert torch.equal(out, torch.full_like(out, 7.0)) and st.phase == ph
        for a, b in zip(states(st), b0):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))

    def refused(**kw):
        def go():
            assert raw(**kw) == -1 and L.gtcrn_last_error()
        nothing_ran(go)

    refused(hb=None)                                                # NULL high-band state
    refused(gain=None)                                              # NULL gains
    refused(hb=st.hb.data_ptr() + 4)                                # off the 16-byte grid
    refused(xp=out.data_ptr())                                      # in place
    refused(xp=big.data_ptr(), xs=2 * n, op=big.data_ptr() + 4 * (n - 1), os_=2 * n)      # rows interleaved, one sample shared

    def in_place():
        with pytest.raises(GtcrnError):
            eng.packet_stream_step(st, x, out=x)
    nothing_ran(in_place)
    ss = eng.new_packet_slot_state(S, win, n, fs, max_active=M, highband=0.5)

    def slots_in_place():
        with pytest.raises(GtcrnError):
            eng.packet_stream_step_slots(ss, i32([0, 1, 2]), x, out=x)
    got = _launches(eng, slots_in_place)
    assert not any(got.values()) and not ss.hb.any() and not ss.phase.any()
    assert L.gtcrn_packet_stream_step_slots_hb(ss._h, ss.model.data_ptr(), ss.wave.data_ptr(), ss.pkt.data_ptr(),
                                               ss.phase.data_ptr(), i32([0, 1, 2]).data_ptr(), None, M, x.data_ptr(), n,
                                               out.data_ptr(), n, ss.window.data_ptr(), None, ss.hb_gain.data_ptr(), sp) == -1
    assert L.gtcrn_packet_stream_hb_reset(st._h, None, 1, sp) == -1
    assert L.gtcrn_packet_stream_hb_reset(st._h, st.hb.data_ptr(), N + 1, sp) == -1
    assert L.gtcrn_packet_stream_hb_reset_slots(ss._h, ss.hb.data_ptr(), None, None, M, sp) == -1
    plain16 = eng.new_packet_state(N, win, 160, 16000)              # a handle whose (fs, n) has no high band
    x16 = torch.zeros(N, 160, device="cuda")
    assert L.gtcrn_packet_stream_step_hb(plain16._h, plain16.model.data_ptr(), plain16.wave.data_ptr(), plain16.pkt.data_ptr(),
                                         x16.data_ptr(), 160, out.data_ptr(), 160, N, plain16.window.data_ptr(),
                                         st.hb.data_ptr(), st.hb_gain.data_ptr(), sp) == -1
    assert b"high band" in L.gtcrn_last_error() and plain16.phase == 0 and not plain16.pkt.any()
