"""The level meters (include/gtcrn_micro_hip.h, "level meters") on every live waveform path: per stream a record
{E_dry, E_out, peak, blocks} advanced by the synthesis kernel.  The checker (tests/meter_checker.py) holds float64 sums of
the emitted float blocks and of the dry blocks aligned with them, with the derived bound of the stated reduction depth;
the records are also compared bit for bit with the numpy float32 emulation of the stated order, and with each other
across partitions, forms and a captured graph.  Outputs and states must equal those of an unmetered state stepped
alongside."""
import numpy as np
import pytest

from conftest import load_params
import meter_checker as MC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

G6, G12 = 10.0 ** (-6 / 20), 10.0 ** (-12 / 20)
GAINS = [0.0, 1.0, G6, G12, 0.3718]            # as in the dry-gain tests
SENT = 7.25                                    # fills records no call may touch


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


def blocks(t):
    """(N, 256 K) tensor -> numpy (N, K, 256) float32."""
    a = t.detach().cpu().numpy().astype(np.float32)
    return a.reshape(a.shape[0], -1, 256)


def records(st):
    return st.meters.detach().cpu().numpy().copy()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def dry_of(x):
    """The dry blocks of a stream stepped from its reset: the input one hop late, zeros for the structural zero block."""
    xb = blocks(x)
    return np.concatenate([np.zeros_like(xb[:, :1]), xb[:, :-1]], 1)


def five_streams(K, seed=1):
    """The inputs of case 1: noise at 0.1; zeros; noise whose largest sample is negative; the same kind (stepped in bypass, so
    the largest OUTPUT sample is negative too); noise at amplitude 3."""
    x = noise(5, 256 * K, seed)
    x[1] = 0
    x[2, 256 * 3 + 41] = -0.95
    x[3, 256 * 2 + 17] = -0.9
    x[4] *= 30
    return x


def step_calls(eng, st, x, calls, plain=None, each=None):
    """x (N, 256 K) through wave_stream_step in calls of `calls` hops; plain: an unmetered state stepped alongside, outputs
    and both states must stay equal; each(k0, k1, out): runs after the call over hops k0..k1-1."""
    outs, k = [], 0
    for nh in calls:
        xin = x[:, 256 * k:256 * (k + nh)]
        out = eng.wave_stream_step(st, xin)
        if plain is not None:
            assert torch.equal(out, eng.wave_stream_step(plain, xin)), k
            assert torch.equal(st.wave, plain.wave) and torch.equal(st.model, plain.model), k
        if each is not None:
            each(k, k + nh, out)
        outs.append(out)
        k += nh
    assert 256 * k == x.shape[1]
    return torch.cat(outs, 1)


# ------------------------------------------------------------------------------------------------------- 1. hop form
def test_hop_form_against_the_checker(eng, win):
    N, K, calls = 5, 10, [1, 2, 3, 1, 3]
    x = five_streams(K)
    gains = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], device="cuda")
    dry = dry_of(x)

    def states():
        a, b = eng.new_wave_state(N, win, meters=True), eng.new_wave_state(N, win)
        a.set_dry_gain(gains)
        b.set_dry_gain(gains.clone())
        return a, b
    # per call: the records are zeroed before every call (K <= 3 in the bound)
    st, plain = states()
    assert st.meters.shape == (N, 4) and st.meters.dtype == torch.float32 and not st.meters.any() and plain.meters is None

    def per_call(k0, k1, out):
        rec, ob = records(st), blocks(out)
        for s in range(N):
            print(f"call hops {k0}..{k1 - 1} stream {s}: record {rec[s].tolist()} "
                  f"reference {MC.reference(ob[s], dry[s, k0:k1])}")
            MC.check(rec[s], ob[s], dry[s, k0:k1], what=(k0, s))
            assert MC.same_bits(rec[s], MC.emulate(ob[s], dry[s, k0:k1])), (k0, s)
        st.reset_meters()
    step_calls(eng, st, x, calls, plain, per_call)
    # accumulated: zeroed once
    st, plain = states()
    out = step_calls(eng, st, x, calls, plain)
    rec, ob = records(st), blocks(out)
    for s in range(N):
        print(f"accumulated stream {s}: record {rec[s].tolist()} reference {MC.reference(ob[s], dry[s])}")
        MC.check(rec[s], ob[s], dry[s], K=K, what=s)
        assert MC.same_bits(rec[s], MC.emulate(ob[s], dry[s])), s
    assert (rec[:, 3] == K).all()
    assert MC.same_bits(rec[1], np.array([0, 0, 0, K], np.float32))                      # silence: exactly zero
    assert rec[0, 1] > 0 and rec[0, 1] != rec[0, 0]
    assert float(rec[2, 2]) == float(np.abs(ob[2]).max())
    assert rec[3, 2] == np.float32(0.9) == -ob[3].min() and ob[3].max() < np.float32(0.9)        # the peak is of |y|
    # bypass: the output is the dry signal, both energies are the same bits and the checker's dry energy
    assert MC.same_bits(rec[3, 0:1], rec[3, 1:2]) and not ob[3, 0].any() and (ob[3, 1:] == blocks(x)[3, :-1]).all()
    assert abs(float(rec[3, 1]) - MC.reference(ob[3], dry[3])[0]) <= MC.bound(K) * MC.reference(ob[3], dry[3])[0]
    assert rec[4, 2] > 1.0                                                               # the clip indicator


# --------------------------------------------------------------------------------------------------- 2. lane coverage
@pytest.mark.parametrize("calls", [[2], [1, 1]])
def test_every_lane_position_is_metered(eng, win, calls):
    pos = [0, 1, 126, 127, 128, 129, 254, 255]
    N = len(pos)
    x = torch.zeros(N, 512, device="cuda")
    for s, p in enumerate(pos):
        x[s, p] = 0.5
    st, plain = eng.new_wave_state(N, win, meters=True), eng.new_wave_state(N, win)
    out = step_calls(eng, st, x, calls, plain)
    rec, ob = records(st), blocks(out)
    for s in range(N):
        assert float(rec[s, 0]) == 0.25 and float(rec[s, 3]) == 2.0, (s, rec[s])
        assert MC.same_bits(rec[s, 2:3], np.abs(ob[s]).max(keepdims=True).reshape(1)), (s, rec[s])
        MC.check(rec[s], ob[s], dry_of(x)[s], what=s)


# ---------------------------------------------------------------------------------------------- 3. partition invariance
def test_records_do_not_depend_on_the_partition(eng, win):
    N, K = 5, 12
    x = noise(N, 256 * K, 3)
    recs = []
    for calls in ([1] * 12, [3] * 4, [6, 6]):
        st = eng.new_wave_state(N, win, meters=True)
        step_calls(eng, st, x, calls)
        recs.append(st.meters.clone())
    assert torch.equal(bits(recs[0]), bits(recs[1])) and torch.equal(bits(recs[0]), bits(recs[2]))
    assert torch.equal(recs[0], recs[1]) and torch.equal(recs[0], recs[2])
    assert (recs[0][:, 3] == K).all() and (recs[0][:, :3] > 0).all()
    # the slot form: 9 resident slots, 5 of them step, in a permuted table of 6 rows of which the device count admits 5
    S, table = 9, [7, 2, 8, 0, 5, 3]
    st = eng.new_wave_state(S, win, meters=True)
    st.meters.fill_(SENT)
    for s in table[:N]:
        st.reset_meters(s, s + 1)
    count = i32([N])
    for k in range(K):
        xin = torch.zeros(6, 256, device="cuda")
        xin[:N] = x[:, 256 * k:256 * (k + 1)]
        eng.wave_stream_step_slots(st, i32(table), xin, count=count)
    got = st.meters
    assert torch.equal(bits(got[table[:N]]), bits(recs[0]))
    idle = [s for s in range(S) if s not in table[:N]]
    assert 3 in idle and len(idle) == 4
    assert torch.equal(bits(got[idle]), bits(torch.full((4, 4), SENT)))                  # idle slots and the row beyond the count


# -------------------------------------------------------------------------------------------------------- 4. PCM16
def test_pcm16_form_meters_the_float_before_the_rounding(eng, win):
    from gtcrn_micro_amd import pcm16_to_f32
    N, K, calls = 5, 9, [1, 2, 3, 3]
    x16 = (noise(N, 256 * K + 96, 4, 9000)).round().clamp(-32768, 32767).to(torch.int16)
    xf = pcm16_to_f32(x16.contiguous())
    g = torch.tensor([0.0, 1.0, G6, 0.0, G12], device="cuda")
    sa, sb = eng.new_wave_state(N, win, meters=True), eng.new_wave_state(N, win, meters=True)
    sa.set_dry_gain(g)
    sb.set_dry_gain(g.clone())
    step_calls(eng, sa, x16[:, :256 * K], calls)
    of = step_calls(eng, sb, xf[:, :256 * K], calls)
    assert torch.equal(bits(sa.meters), bits(sb.meters)) and (sa.meters[:, 3] == K).all()
    rec = records(sb)
    for s in range(N):
        MC.check(rec[s], blocks(of)[s], dry_of(xf[:, :256 * K])[s], what=s)
    eng.wave_stream_flush(sa, x16[:, 256 * K:])
    eng.wave_stream_flush(sb, xf[:, 256 * K:])
    assert torch.equal(bits(sa.meters), bits(sb.meters)) and (sa.meters[:, 3] == K + 1).all()


# --------------------------------------------------------------------------------------------------------- 5. flush
@pytest.mark.parametrize("r", [0, 100])
def test_flush_counts_one_block_with_the_ring_as_dry(eng, win, r):
    N, K = 5, 4
    x = noise(N, 256 * K + r, 50 + r)
    st, plain = eng.new_wave_state(N, win, meters=True), eng.new_wave_state(N, win)
    step_calls(eng, st, x[:, :256 * K], [3, 1], plain)
    st.reset_meters()
    last = eng.wave_stream_flush(st, x[:, 256 * K:])
    assert torch.equal(last, eng.wave_stream_flush(plain, x[:, 256 * K:]))
    assert torch.equal(st.wave, plain.wave) and torch.equal(st.model, plain.model)
    rec, ring = records(st), blocks(x[:, 256 * (K - 1):256 * K])
    for s in range(N):
        assert rec[s, 3] == 1.0
        MC.check(rec[s], blocks(last)[s], ring[s], what=s)
        assert MC.same_bits(rec[s], MC.emulate(blocks(last)[s], ring[s])), s


def test_flush_of_a_short_stream_counts_one_zero_block(eng, win):
    N = 3
    x = noise(N, 256, 6) + 0.5
    st = eng.new_wave_state(N, win, meters=True)
    assert not eng.wave_stream_step(st, x).any()
    st.reset_meters()
    assert not eng.wave_stream_flush(st, x[:, :0]).any()            # 256 samples in all: no block
    assert MC.same_bits(records(st), np.tile(np.array([0, 0, 0, 1], np.float32), (N, 1)))
    st2 = eng.new_wave_state(N, win, meters=True)
    assert not eng.wave_stream_flush(st2, x[:, :200]).any()
    assert MC.same_bits(records(st2), np.tile(np.array([0, 0, 0, 1], np.float32), (N, 1)))


# ------------------------------------------------------------------------------------------------- 6. with the limit
def test_limited_output_is_what_is_metered(eng, win):
    N, K, calls = 5, 8, [1, 2, 5]
    x = noise(N, 256 * K, 7)
    g = torch.tensor(GAINS, dtype=torch.float32, device="cuda")
    sl, pl = eng.new_wave_state(N, win, meters=True), eng.new_wave_state(N, win)
    sl.set_dry_gain(g)
    pl.set_dry_gain(g.clone())
    out = step_calls(eng, sl, x, calls, pl)
    sn = eng.new_wave_state(N, win, meters=True)
    outn = step_calls(eng, sn, x, calls, eng.new_wave_state(N, win))
    rec, recn, dry = records(sl), records(sn), dry_of(x)
    for s in range(N):
        MC.check(rec[s], blocks(out)[s], dry[s], what=s)
        MC.check(recn[s], blocks(outn)[s], dry[s], what=s)
        assert MC.same_bits(rec[s], MC.emulate(blocks(out)[s], dry[s])), s
    assert MC.same_bits(rec[0], recn[0])                             # beta = 0: the record of the run without gains
    assert MC.same_bits(rec[1, 0:1], rec[1, 1:2])                    # beta = 1
    assert MC.same_bits(rec[:, 0], recn[:, 0]) and not MC.same_bits(rec[2:, 1], recn[2:, 1])


# ---------------------------------------------------------------------------------------------------- 7. packet forms
@pytest.mark.parametrize("fs,n", [(16000, 160), (16000, 320), (48000, 480)])
def test_packet_form_against_the_handoffs(eng, win, fs, n):
    N = 5
    st, plain = eng.new_packet_state(N, win, n, fs, meters=True), eng.new_packet_state(N, win, n, fs)
    P = st.period
    x = noise(N, n * P, fs + n)
    x[1] = 0
    carry = np.zeros((N, 1, 256), np.float32)         # the dry block of the next call's first hop (zeros: the stream's first)
    seen, total = set(), 0
    for c in range(P):
        h = st.next_hops
        seen.add(h)
        st.meters.fill_(SENT) if h == 0 else st.reset_meters()
        xin = x[:, n * c:n * (c + 1)]
        assert torch.equal(eng.packet_stream_step(st, xin), eng.packet_stream_step(plain, xin)), c
        assert torch.equal(st.wave, plain.wave) and torch.equal(st.model, plain.model) and torch.equal(st.pkt, plain.pkt), c
        if h == 0:
            assert torch.equal(bits(st.meters), bits(torch.full((N, 4), SENT))), c          # no hop: not touched
            continue
        a16, b16 = blocks(eng.packet_stream_handoff(st, 0)), blocks(eng.packet_stream_handoff(st, 1))
        assert a16.shape == b16.shape == (N, h, 256)
        dry = np.concatenate([carry, a16[:, :-1]], 1)
        rec = records(st)
        for s in range(N):
            MC.check(rec[s], b16[s], dry[s], what=(c, s))
            assert MC.same_bits(rec[s], MC.emulate(b16[s], dry[s])), (c, s)
        assert MC.same_bits(rec[1], np.array([0, 0, 0, h], np.float32)), c
        carry = a16[:, -1:]
        total += h
    assert seen == ({0, 1} if n16(fs, n) == 160 else {1, 2}) and total == n16(fs, n) * P // 256


def n16(fs, n):
    return n * 16000 // fs


def test_rate_form_against_the_handoffs(eng, win):
    N, H = 5, 128
    st, plain = eng.new_rate_state(N, win, 8000, meters=True), eng.new_rate_state(N, win, 8000)
    x = noise(N, H * 5, 8)
    carry, k = np.zeros((N, 1, 256), np.float32), 0
    for nh in (2, 3):
        xin = x[:, H * k:H * (k + nh)]
        st.reset_meters()
        assert torch.equal(eng.rate_stream_step(st, xin), eng.rate_stream_step(plain, xin))
        assert torch.equal(st.wave, plain.wave) and torch.equal(st.model, plain.model) and torch.equal(st.rate, plain.rate)
        a16, b16 = blocks(eng.rate_stream_handoff(st, nh, 0)), blocks(eng.rate_stream_handoff(st, nh, 1))
        dry = np.concatenate([carry, a16[:, :-1]], 1)
        rec = records(st)
        for s in range(N):
            MC.check(rec[s], b16[s], dry[s], what=(k, s))
            assert MC.same_bits(rec[s], MC.emulate(b16[s], dry[s])), (k, s)
        carry = a16[:, -1:]
        k += nh


def test_packet_slots_equal_one_stream_groups(eng, win):
    """16 kHz / 320: a call steps 1 or 2 hops per slot, as one or two 1-hop rounds of the indexed step; a one-stream packet
    state makes the 2-hop contiguous call.  Nine slots on a ragged 12-tick schedule."""
    S, n, T = 9, 320, 12
    rng = np.random.default_rng(9)
    st = eng.new_packet_slot_state(S, win, n, meters=True)
    plain = eng.new_packet_slot_state(S, win, n)
    singles = [eng.new_packet_state(1, win, n, meters=True) for _ in range(S)]
    x = noise(S, n * T, 9)
    fed = [0] * S
    for t in range(T):
        act = [s for s in rng.permutation(S) if rng.random() < 0.6] or [int(rng.integers(S))]
        if t == 0:
            act = list(rng.permutation(S))                  # everyone has at least one packet
        xin = torch.stack([x[s, n * fed[s]:n * (fed[s] + 1)] for s in act])
        got = eng.packet_stream_step_slots(st, i32(act), xin)
        assert torch.equal(got, eng.packet_stream_step_slots(plain, i32(act), xin)), t
        for i, s in enumerate(act):
            assert torch.equal(got[i:i + 1], eng.packet_stream_step(singles[s], xin[i:i + 1])), (t, s)
            fed[s] += 1
        assert torch.equal(st.wave, plain.wave) and torch.equal(st.model, plain.model) and torch.equal(st.pkt, plain.pkt), t
    want = torch.cat([u.meters for u in singles])
    assert torch.equal(bits(st.meters), bits(want))
    assert sorted(set(fed)) != [T] and (want[:, 3] == torch.tensor([f * n // 256 for f in fed], device="cuda")).all()
    assert (want[:, 3] >= 1).all() and (want[:, 1] > 0).any()


# ------------------------------------------------------------------------------------------------ 8. one captured graph
def test_one_captured_graph_meters_a_changing_active_set(eng, win):
    S, M, T = 9, 6, 8
    rng = np.random.default_rng(10)
    x = noise(S, 256 * T, 10)
    ticks = [(rng.permutation(S)[:M], int(c)) for c in (6, 3, 0, 5, 6, 1, 4, 6)]
    seen, inputs = [0] * S, []
    for perm, c in ticks:
        xin = torch.zeros(M, 256, device="cuda")
        for i in range(c):
            s = int(perm[i])
            xin[i] = x[s, 256 * seen[s]:256 * (seen[s] + 1)]
            seen[s] += 1
        inputs.append(xin)
    se = eng.new_wave_state(S, win, meters=True)
    eager = []
    for k, ((p, c), xin) in enumerate(zip(ticks, inputs)):
        if k % 4 == 0:
            se.reset_meters()
        eng.wave_stream_step_slots(se, i32(p), xin, count=i32([c]))
        eager.append(se.meters.clone())
    sg = eng.new_wave_state(S, win, meters=True)
    eng.reserve(M, 1)
    slots, count = i32(ticks[0][0]), i32([0])
    xin, out = torch.zeros(M, 256, device="cuda"), torch.zeros(M, 256, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.wave_stream_step_slots(sg, slots, xin, count=count, out=out)         # warm-up with count 0: nothing steps
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.wave_stream_step_slots(sg, slots, xin, count=count, out=out)
    assert not sg.meters.any()
    # a step through a state without meters clears the model's pointer: the graph holds the address all the same
    eng.wave_stream_step(eng.new_wave_state(2, win), x[:2, :256])
    for k, ((p, c), xk) in enumerate(zip(ticks, inputs)):
        if k % 4 == 0:
            sg.reset_meters()                                                    # a memset outside the graph
        slots.copy_(i32(p))
        count.fill_(c)
        xin.copy_(xk)
        graph.replay()
        assert torch.equal(bits(sg.meters), bits(eager[k])), k
    assert torch.equal(sg.model, se.model) and torch.equal(sg.wave, se.wave)
    assert eager[-1][:, 3].sum() == sum(c for _, c in ticks[4:])


# ----------------------------------------------------------------------------------------------------- 9. launch records
def _launches(eng, fn):
    eng.timing_enable(True)
    fn()
    torch.cuda.synchronize()
    t = {k: v[1] for k, v in eng.timing_read().items()}
    eng.timing_enable(False)
    return t


def test_a_metered_call_makes_the_launches_of_its_plain_form(eng, win):
    assert eng.kernel_names()[-1] == "k_wave_synthesis_meter"
    N = 8
    x = noise(N, 256 * 3, 12)

    def swapped(rec, a):
        rec = dict(rec)
        rec["k_wave_synthesis_meter"] = rec.pop(a)
        return rec
    for db, plain_name in ((None, "k_wave_synthesis"), (6, "k_wave_synthesis_mix")):
        for nh in (1, 3):
            sp, sm = eng.new_wave_state(N, win, atten_lim_db=db), eng.new_wave_state(N, win, atten_lim_db=db, meters=True)
            plain = _launches(eng, lambda: eng.wave_stream_step(sp, x[:, :256 * nh]))
            met = _launches(eng, lambda: eng.wave_stream_step(sm, x[:, :256 * nh]))
            assert plain[plain_name] == 1 and met == swapped(plain, plain_name), (db, nh)
            if nh == 1:
                assert sum(met.values()) == 3
            plain = _launches(eng, lambda: eng.wave_stream_flush(sp, x[:, :17]))
            met = _launches(eng, lambda: eng.wave_stream_flush(sm, x[:, :17]))
            assert met == swapped(plain, plain_name) and sum(met.values()) == 3
    sm = eng.new_wave_state(N, win, meters=True)
    eng.wave_stream_step(sm, x[:, :256])
    before = sm.meters.clone()
    assert (before[:, 3] == 1).all()
    # a state without meters on the same engine: the plain names are back, the earlier records stay
    sp = eng.new_wave_state(N, win)
    got = _launches(eng, lambda: eng.wave_stream_step(sp, x[:, :256]))
    assert got.get("k_wave_synthesis") == 1 and "k_wave_synthesis_meter" not in got
    rp = eng.new_rate_state(N, win, 48000)
    got = _launches(eng, lambda: eng.rate_stream_step(rp, x[:, :768]))
    assert got.get("k_wave_synthesis") == 1 and "k_wave_synthesis_meter" not in got
    rm = eng.new_rate_state(N, win, 48000, meters=True)
    assert _launches(eng, lambda: eng.rate_stream_step(rm, x[:, :768])) == swapped(got, "k_wave_synthesis")
    pp, pm = eng.new_packet_state(N, win, 320), eng.new_packet_state(N, win, 320, meters=True)
    plain = _launches(eng, lambda: eng.packet_stream_step(pp, x[:, :320]))
    assert _launches(eng, lambda: eng.packet_stream_step(pm, x[:, :320])) == swapped(plain, "k_wave_synthesis")
    eng.packet_stream_step(pp, x[:, :320])
    assert torch.equal(bits(sm.meters), bits(before))


def test_setter_rejects_a_misaligned_pointer(eng, win):
    from gtcrn_micro_amd._lib import lib
    buf = torch.zeros(9, device="cuda")
    assert lib().gtcrn_wave_stream_set_meters(eng._h, buf.data_ptr() + 4) == -1
    assert b"16-byte aligned" in lib().gtcrn_last_error()
    assert lib().gtcrn_wave_stream_set_meters(eng._h, buf.data_ptr()) == 0
    assert lib().gtcrn_wave_stream_set_meters(eng._h, None) == 0


# ----------------------------------------------------------------------------------------------------------- 10. levels
def test_levels_are_rfc6464_of_the_record(eng, win):
    from gtcrn_micro_amd import GtcrnError, level_dbov
    from gtcrn_micro_amd.streaming.gtcrn_micro_stream import StreamGTCRNMicro
    K = 4
    x = five_streams(K, seed=13)
    st = eng.new_wave_state(5, win, meters=True)
    step_calls(eng, st, x, [2, 2])
    rec = records(st).astype(np.float64)
    lv = st.levels()
    assert lv.shape == (5,) and lv.tolist() == [level_dbov(rec[s, 1], 256 * rec[s, 3]) for s in range(5)]
    assert lv[1] == 127 and 0 <= lv[4] < lv[0] < 127
    st.reset_meters(0, 1)
    assert st.levels()[0] == 127 and st.levels()[4] == lv[4]
    with pytest.raises(GtcrnError):
        eng.new_wave_state(5, win).levels()
    with pytest.raises(GtcrnError):
        eng.new_wave_state(5, win).reset_meters()
    stream = StreamGTCRNMicro().cuda().eval()
    assert stream.init_wave_state(2, win, meters=True).meters.shape == (2, 4) and stream.init_wave_state(2, win).meters is None
    assert stream.init_wave_state(2, win, fs=48000, meters=True).meters.shape == (2, 4)
    assert stream.init_wave_state(2, win, packet=160, meters=True).meters.shape == (2, 4)
    assert stream.init_wave_state(3, win, packet=160, resident=True, meters=True).meters.shape == (3, 4)
