"""The level control (include/gtcrn_micro_hip.h, "level control") on every live waveform path.  The checker
(tests/alc_checker.py) is the contract in numpy float32; a twin state WITHOUT level control, fed the same input, supplies the
wet blocks w (and, with gains, the mixed blocks m), because its outputs are what the other test files pin.  theta is set to
the median of the twin run's block E_w and c to half its largest peak, so speech / non-speech and limited / unlimited blocks
both occur by construction; every test asserts from the checker's trace that they did.  Every comparison is exact."""
import numpy as np
import pytest

from conftest import load_params
import alc_checker as AK
import meter_checker as MC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
FFT_WAVES = 4                                                 # streams that share a synthesis workgroup
BASE = dict(hang_ms=32, ratio_db=-60, rise_db_s=300, fall_db_s=600, target_dbov=-20, min_gain_db=-12, max_gain_db=30)
MIXED = {"speech", "silence", "hangover", "hangover_ends", "limited", "unlimited", "zero"}


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


def npf(t):
    return t.detach().cpu().numpy().astype(np.float32) if isinstance(t, torch.Tensor) else np.asarray(t, np.float32)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(a, b):
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    if not isinstance(b, torch.Tensor):
        b = torch.from_numpy(np.ascontiguousarray(b, np.float32))
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def stepped(N, K, seed, scale=1.0):
    """Seeded noise whose amplitude steps between 0.3, 1e-3 and exact zeros every three blocks, the streams offset against
    each other by one block."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(N, K, 256, device="cuda", generator=gen)
    amp = torch.tensor([[(0.3, 1e-3, 0.0)[((k + s) // 3) % 3] for k in range(K)] for s in range(N)], device="cuda")
    return (x * amp[:, :, None] * scale).reshape(N, 256 * K)


def delayed(x):
    """The dry samples under the blocks of a stream stepped from its reset: the input one hop late."""
    return np.concatenate([np.zeros_like(x[:, :256]), x[:, :-256]], 1)


def blocks(a):
    a = np.asarray(a, np.float32)
    return a.reshape(a.shape[0], -1, 256)


def tuned(w, m, first=1, **kw):
    """The parameter words of BASE with theta = the median block E_w and c = half the largest |m| of the twin run
    (structural zero blocks left out)."""
    from gtcrn_micro_amd import alc_params
    p = alc_params(**dict(BASE, **kw))
    wb, mb = blocks(w)[:, first:], blocks(m)[:, first:]
    p[0] = F32(np.median([AK.hop_sum(b) for s in wb for b in s]))
    p[9] = F32(0.5) * F32(np.abs(mb).max())
    assert p[0] > 0 and p[9] > 0
    return p


def probed(eng, win, x, **kw):
    """tuned() on the blocks a plain hop-form state emits for x (N, 256 K): the words for a form whose wave step sees the same
    stream."""
    w = npf(eng.wave_stream_step(eng.new_wave_state(x.shape[0], win), x))
    return tuned(w, w, **kw)


def put(st, params):
    st.alc_params.copy_(torch.from_numpy(np.asarray(params, np.float32)))


def expect(params, w, x, m, first=0, rec0=None):
    """The checker for N streams: w, x, m (N, 256 K) numpy -> y (N, 256 K), records (N, K, 8), the union of the traces."""
    ys, recs, seen = [], [], set()
    for s in range(len(w)):
        y, r, tr = AK.stream(params, blocks(w)[s], blocks(x)[s], blocks(m)[s], first, None if rec0 is None else rec0[s])
        ys.append(y.reshape(-1))
        recs.append(r)
        seen |= AK.seen(tr)
    return np.stack(ys), np.stack(recs), seen


def run_hops(eng, st, x, hops, each=None):
    outs, k = [], 0
    for c, h in enumerate(hops):
        if each is not None:
            each(c, k)
        outs.append(eng.wave_stream_step(st, x[:, 256 * k:256 * (k + h)]))
        k += h
    return torch.cat(outs, 1)


HOPS = [1, 2, 3, 1, 1, 2, 3, 2, 1, 3]                         # 10 calls, 19 blocks: the hangover of 2 expires many times


# ------------------------------------------------------------------------------------------------------ 1. hop form
@pytest.mark.parametrize("N", [1, FFT_WAVES - 1, FFT_WAVES + 2])
@pytest.mark.parametrize("pcm", [False, True])
def test_hop_form_equals_the_checker(eng, win, N, pcm):
    """Outputs, the records after every call, state.voice() and both state tensors; the int16 form is the float form
    between the conversions (one rounding, of y)."""
    from gtcrn_micro_amd import pcm16_to_f32, f32_to_pcm16
    K = sum(HOPS)
    if pcm:
        x16 = stepped(N, K, 40 + N, 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        xf = pcm16_to_f32(x16.contiguous())
    else:
        xf = stepped(N, K, 40 + N)
    xin = x16 if pcm else xf
    plain, plain_in = eng.new_wave_state(N, win), eng.new_wave_state(N, win)
    w = npf(run_hops(eng, plain, xf, HOPS))
    run_hops(eng, plain_in, xin, HOPS)
    params = tuned(w, w)
    want, recs, seen = expect(params, w, delayed(npf(xf)), w)
    assert MIXED | {"first_estimate", "smoothed"} <= seen, sorted(MIXED - seen)
    st = eng.new_wave_state(N, win, alc=BASE)
    assert tuple(st.alc.shape) == (N, 8) and tuple(st.alc_params.shape) == (16,) and same(st.alc, np.tile(AK.INIT, (N, 1)))
    put(st, params)
    done = []

    def after_previous(c, k):
        if k:
            assert same(st.alc, recs[:, k - 1]), c
            assert st.voice().dtype == torch.bool and st.voice().tolist() == (recs[:, k - 1, 3] != 0).tolist(), c
        done.append(k)

    got = run_hops(eng, st, xin, HOPS, after_previous)
    assert same(st.alc, recs[:, -1]) and len(done) == len(HOPS)
    want = torch.from_numpy(want).cuda()
    assert torch.equal(got, f32_to_pcm16(want.contiguous())) if pcm else same(got, want)
    assert torch.equal(st.wave, plain_in.wave) and torch.equal(st.model, plain_in.model)
    assert not same(got, run_hops(eng, eng.new_wave_state(N, win), xin, HOPS))        # the gain is seen
    db = st.alc_gain_db()
    assert db.shape == (N,) and np.allclose(db, 20 * np.log10(recs[:, -1, 0].astype(np.float64)))


# ------------------------------------------------------------------------------ 2. gains, ramps and meters compose
def test_gains_ramps_and_meters_compose(eng, win):
    """m is the ramped mix of the twin with the same gains; the meters see y, their E_dry stays the dry block's."""
    N, K = 6, sum(HOPS)
    x = stepped(N, K, 50)
    rng = np.random.default_rng(50)
    gains = [[(None, 0, 6, 12, 3, 20)[int(i)] for i in rng.integers(0, 6, N)] for _ in HOPS]
    plain = eng.new_wave_state(N, win)
    mixed = eng.new_wave_state(N, win, atten_lim_db=gains[0], ramp=True)
    st = eng.new_wave_state(N, win, atten_lim_db=gains[0], ramp=True, meters=True, alc=BASE)
    w = npf(run_hops(eng, plain, x, HOPS))
    m = npf(run_hops(eng, mixed, x, HOPS, lambda c, k: mixed.set_atten_lim_db(gains[c])))
    assert not same(w, m)
    params = tuned(w, m)
    put(st, params)
    got = run_hops(eng, st, x, HOPS, lambda c, k: st.set_atten_lim_db(gains[c]))
    dry = delayed(npf(x))
    want, recs, seen = expect(params, w, dry, m)
    assert MIXED <= seen, sorted(MIXED - seen)
    assert same(got, want) and same(st.alc, recs[:, -1])
    assert same(st.gain_ramp, mixed.gain_ramp) and same(st.wave, plain.wave) and same(st.model, plain.model)
    rec = npf(st.meters)
    dry[:, :256] = 0                                             # (under the structural zero block the meters take zeros)
    for s in range(N):
        assert MC.same_bits(rec[s], MC.emulate(blocks(want)[s], blocks(dry)[s])), s


# ------------------------------------------------------------------------------------------------- 3. measure only
@pytest.mark.parametrize("kw", [dict(), dict(atten_lim_db=[6, None, 0, 12, 3, 6]), dict(meters=True),
                                dict(atten_lim_db=[6, None, 0, 12, 3, 6], ramp=True)], ids=["plain", "limit", "meters", "limit+ramp"])
def test_vad_mode_leaves_every_bit_alone(eng, win, kw):
    N, K = 6, sum(HOPS)
    x = stepped(N, K, 60)
    st, twin, plain = eng.new_wave_state(N, win, alc="vad", **kw), eng.new_wave_state(N, win, **kw), eng.new_wave_state(N, win)
    assert float(st.alc_params[10]) == 0.0
    moves = lambda s: (lambda c, k: s.set_atten_lim_db(12 if c % 2 else [0, 6, None, 3, 12, 6])) if "atten_lim_db" in kw else None
    w = npf(run_hops(eng, plain, x, HOPS))
    m = run_hops(eng, twin, x, HOPS, moves(twin))
    params = tuned(w, npf(m), mode=0)
    put(st, params)
    got = run_hops(eng, st, x, HOPS, moves(st))
    assert same(got, m) and same(st.wave, twin.wave) and same(st.model, twin.model)
    if kw.get("meters"):
        assert same(st.meters, twin.meters)
    if kw.get("ramp"):
        assert same(st.gain_ramp, twin.gain_ramp)
    want, recs, seen = expect(params, w, delayed(npf(x)), npf(m))
    assert {"mode0", "speech", "silence", "hangover"} <= seen
    assert same(want, m) and same(st.alc, recs[:, -1]) and (recs[:, -1, 0] == 1).all()
    assert 0 < recs[:, -1, 4].sum() < recs[:, -1, 5].sum()


# ------------------------------------------------------------------------------------------- 4. hop cuts and flush
@pytest.mark.parametrize("r", [0, 100])
def test_the_cut_of_hops_does_not_matter_and_the_flush_block_is_a_block(eng, win, r):
    N = 5
    x = stepped(N, 7, 70 + r)[:, :256 * 6 + r] + 1e-4
    plain = eng.new_wave_state(N, win)
    w = npf(torch.cat([eng.wave_stream_step(plain, x[:, :1536]), eng.wave_stream_flush(plain, x[:, 1536:])], 1))
    params = tuned(w, w)
    runs = []
    for cut in ([4], [1, 1, 1, 1], [2, 2]):
        st = eng.new_wave_state(N, win, alc=BASE)
        put(st, params)
        o = [eng.wave_stream_step(st, x[:, :512])]
        o.append(run_hops(eng, st, x[:, 512:1536], cut))
        o.append(eng.wave_stream_flush(st, x[:, 1536:]))
        assert same(st.wave, plain.wave) and same(st.model, plain.model)
        runs.append((torch.cat(o, 1), st.alc.clone()))
    for other in runs[1:]:
        assert same(runs[0][0], other[0]) and same(runs[0][1], other[1])
    dry = np.concatenate([delayed(npf(x[:, :1536])), npf(x[:, 1280:1536])], 1)       # the flush block lies over the ring's newest hop
    want, recs, seen = expect(params, w, dry, w)
    assert {"speech", "limited", "unlimited"} <= seen
    assert same(runs[0][0], want) and same(runs[0][1], recs[:, -1]) and (recs[:, -1, 5] == 6).all()


def test_a_flush_without_a_block_leaves_the_record_alone(eng, win):
    N = 3
    x = stepped(N, 1, 71) + 0.5
    st = eng.new_wave_state(N, win, alc=BASE)
    assert not eng.wave_stream_step(st, x).any() and same(st.alc, np.tile(AK.INIT, (N, 1)))
    mark = torch.arange(8.0 * N, device="cuda").reshape(N, 8) + 0.5
    st.alc.copy_(mark)
    assert not eng.wave_stream_flush(st, x[:, :0]).any()          # 256 samples in all: no block
    assert same(st.alc, mark)
    st2 = eng.new_wave_state(N, win, alc=BASE)
    st2.alc.copy_(mark)
    assert not eng.wave_stream_flush(st2, x[:, :200]).any() and same(st2.alc, mark)


# ---------------------------------------------------------------------------------------------------------- 5. join
def test_a_join_resets_only_the_named_record(eng, win):
    N = 5
    x = stepped(N, 9, 80)
    plain = eng.new_wave_state(N, win)
    w = [eng.wave_stream_step(plain, x[:, :1024])]
    eng.wave_stream_reset_slots(plain, i32([2]))
    w.append(eng.wave_stream_step(plain, x[:, 1024:]))
    # the second half against the checker: stream 2 from a fresh record, the others from theirs
    wn, xn = npf(torch.cat(w, 1)), npf(x)
    params = tuned(wn, wn)
    a, b = eng.new_wave_state(N, win, alc=BASE), eng.new_wave_state(N, win)
    put(a, params)
    got = [eng.wave_stream_step(a, x[:, :1024])]
    eng.wave_stream_step(b, x[:, :1024])
    rec4 = npf(a.alc)
    for s in (a, b):
        eng.wave_stream_reset_slots(s, i32([2]))
    got.append(eng.wave_stream_step(a, x[:, 1024:]))
    want1, recs1, _ = expect(params, wn[:, :1024], delayed(xn[:, :1024]), wn[:, :1024])
    assert same(got[0], want1) and same(rec4, recs1[:, -1])
    dry2 = xn[:, 768:-256].copy()
    rest = [0, 1, 3, 4]
    want2, recs2, seen = expect(params, wn[rest, 1024:], dry2[rest], wn[rest, 1024:], first=4, rec0=rec4[rest])
    assert same(got[1][rest], want2) and same(a.alc[rest], recs2[:, -1])
    want3, recs3, seen3 = expect(params, wn[2:3, 1024:], dry2[2:3], wn[2:3, 1024:], first=0)
    assert "zero" in seen3 and same(got[1][2:3], want3) and same(a.alc[2:3], recs3[:, -1])
    assert rec4[2, 5] == 3 and recs3[0, -1, 5] == 4 and recs2[0, -1, 5] == 8
    assert {"speech", "silence"} <= seen


# --------------------------------------------------------------------------------------------------------- 6. slots
@pytest.mark.parametrize("pcm", [False, True])
def test_slots_step_the_named_and_leave_the_rest_alone(eng, win, pcm):
    """Seven resident streams; after two contiguous hops the calls name slots 5, 1, 3 and, beyond the device count of 3,
    slot 6.  The named slots equal the contiguous form of the same streams, the others keep every bit."""
    from gtcrn_micro_amd import pcm16_to_f32, f32_to_pcm16
    S, K = 7, 8
    if pcm:
        x16 = stepped(S, K, 90, 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        xf = pcm16_to_f32(x16.contiguous())
    else:
        xf = stepped(S, K, 90)
    xin = x16 if pcm else xf
    plain = eng.new_wave_state(S, win)
    w = npf(eng.wave_stream_step(plain, xf))
    params = tuned(w, w)
    want, recs, seen = expect(params, w, delayed(npf(xf)), w)
    assert {"speech", "silence", "limited", "unlimited"} <= seen
    st = eng.new_wave_state(S, win, alc=BASE)
    put(st, params)
    eng.wave_stream_step(st, xin[:, :512])
    table, cnt, named = i32([5, 1, 3, 6]), i32([3]), [5, 1, 3]
    rest = [s for s in range(S) if s not in named]
    st.alc[rest] += 0.25                                         # marks: an idle slot's record is neither read nor written
    before = [t.clone() for t in (st.alc, st.wave, st.model)]
    want = torch.from_numpy(want).cuda()
    for k in range(2, K):
        rows = xin[[5, 1, 3, 6], 256 * k:256 * (k + 1)].contiguous()
        out = torch.full_like(rows, 77)
        eng.wave_stream_step_slots(st, table, rows, count=cnt, out=out)
        assert (out[3] == 77).all()                               # beyond the count: not written
        ref = want[named, 256 * k:256 * (k + 1)].contiguous()
        assert torch.equal(out[:3], f32_to_pcm16(ref)) if pcm else same(out[:3], ref), k
        assert same(st.alc[named], recs[named, k]), k
        for t, b in zip((st.alc, st.wave, st.model), before):
            assert same(t[rest], b[rest]), k


# -------------------------------------------------------------------------------------------------- 7. packet forms
def moving(rec):
    """A record set in which the decision and the gain both moved: no comparison of records is vacuous."""
    rec = npf(rec)
    return 0 < rec[:, 4].sum() < rec[:, 5].sum() and (rec[:, 0] != 1).any()


@pytest.mark.parametrize("n", [160, 320])
def test_packet_group_at_16k_equals_the_hop_form(eng, win, n):
    """The 16 kHz hand-off is the hop stream: a hop-form state with the same words, fed the inbound hand-off, emits the
    outbound one and ends every call with the same records."""
    N, C = 4, 16
    x = stepped(N, n * C // 256, 100 + n)
    st, hop = eng.new_packet_state(N, win, n, 16000, alc=BASE), eng.new_wave_state(N, win, alc=BASE)
    params = probed(eng, win, x)
    put(st, params)
    put(hop, params)
    hops = 0
    for c in range(C):
        h = st.next_hops
        before = st.alc.clone()
        eng.packet_stream_step(st, x[:, n * c:n * (c + 1)].contiguous())
        if h == 0:
            assert same(st.alc, before), c                        # no hop: the records stay
            continue
        a16, b16 = eng.packet_stream_handoff(st, 0), eng.packet_stream_handoff(st, 1)
        assert same(eng.wave_stream_step(hop, a16), b16) and same(st.alc, hop.alc), c
        hops += h
    assert hops == n * C // 256 and moving(st.alc) and same(st.wave, hop.wave)


def test_packet_slots_equal_one_stream_groups(eng, win):
    """Five resident slots on a ragged schedule (so their phases differ); every slot is the one-stream group fed the same
    packets, outputs and records."""
    S, T, n, fs = 5, 12, 320, 16000
    rng = np.random.default_rng(110)
    st = eng.new_packet_slot_state(S, win, n, fs, alc=BASE)
    singles = [eng.new_packet_state(1, win, n, fs, alc=BASE) for _ in range(S)]
    x = stepped(S, n * T // 256 + 1, 111)
    params = probed(eng, win, x)
    for u in [st] + singles:
        put(u, params)
    fed = [0] * S
    phases = set()
    for t in range(T):
        act = [int(s) for s in rng.permutation(S) if rng.random() < 0.6] or [int(rng.integers(S))]
        if t == 0:
            act = [int(s) for s in rng.permutation(S)]
        xin = torch.stack([x[s, n * fed[s]:n * (fed[s] + 1)] for s in act])
        got = eng.packet_stream_step_slots(st, i32(act), xin)
        for i, s in enumerate(act):
            assert same(got[i:i + 1], eng.packet_stream_step(singles[s], xin[i:i + 1])), (t, s)
            fed[s] += 1
        assert same(st.alc, torch.cat([u.alc for u in singles])), t
        phases.add(tuple(st.phase.tolist()))
    assert any(len(set(q)) > 1 for q in phases) and len(set(fed)) > 1 and moving(st.alc)


# ------------------------------------------------------------------------------------- 8. G.711 and the rate form
def handoffs(eng, st, plain, step, handoff, calls):
    a16, b16, w16 = [], [], []
    for c in calls:
        h = step(st, c)
        if h:                                                     # (the rate form's hand-off buffers belong to the engine:
            a16.append(handoff(st, h, 0))                         # read before the twin steps)
            b16.append(handoff(st, h, 1))
        step(plain, c)
        if h:
            w16.append(handoff(plain, h, 1))
        assert same(st.wave, plain.wave) and same(st.model, plain.model)
    return (npf(torch.cat(v, 1)) for v in (a16, b16, w16))


def test_g711_form_through_its_16k_handoff(eng, win):
    """8 kHz / 160 mu-law: the wave step's hand-off is the checker's stream; the codes are E_law of the float form's output."""
    from gtcrn_micro_amd import g711_to_f32, f32_to_g711
    fs, n, N, C = 8000, 160, 3, 16
    codes = f32_to_g711(stepped(N, n * C // 256 + 1, 120)[:, :n * C].contiguous(), "ulaw")
    xf = g711_to_f32(codes.contiguous(), "ulaw")
    plain = eng.new_packet_state(N, win, n, fs)

    def step(s, c, feed=lambda t: t):
        h = s.next_hops
        s.out.append(eng.packet_stream_step(s, feed(xf[:, n * c:n * (c + 1)].contiguous())))
        return h
    plain.out = []
    hand = lambda s, h, which: eng.packet_stream_handoff(s, which)
    probe = eng.new_packet_state(N, win, n, fs)
    probe.out = []
    _, w16p, _ = handoffs(eng, probe, plain, step, hand, range(C))
    params = tuned(w16p, w16p, first=1)
    runs = {}
    for law in (None, "ulaw"):
        st, tw = eng.new_packet_state(N, win, n, fs, alc=BASE, g711=law), eng.new_packet_state(N, win, n, fs)
        put(st, params)
        st.out, tw.out = [], []
        feed = (lambda t: f32_to_g711(t, "ulaw")) if law else (lambda t: t)
        stp = lambda s, c: step(s, c, feed if s is st else (lambda t: t))
        a16, b16, w16 = handoffs(eng, st, tw, stp, hand, range(C))
        runs[law] = (a16, b16, torch.cat(st.out, 1), st.alc.clone())
        want, recs, seen = expect(params, w16, delayed(a16), w16)
        assert {"speech", "silence", "limited", "unlimited"} <= seen
        assert same(b16, want) and same(st.alc, recs[:, -1]), law
    assert runs["ulaw"][2].dtype == torch.uint8 and same(runs["ulaw"][1], runs[None][1]) and same(runs["ulaw"][3], runs[None][3])
    assert torch.equal(runs["ulaw"][2], f32_to_g711(runs[None][2].contiguous(), "ulaw"))


def test_rate_form_through_its_16k_handoff(eng, win):
    fs, H, N = 48000, 768, 4
    calls = [1, 2, 1, 3, 2, 3]
    x = stepped(N, sum(calls) * 3, 130)
    offs = np.concatenate([[0], np.cumsum(calls)])

    def step(s, c):
        eng.rate_stream_step(s, x[:, H * offs[c]:H * offs[c + 1]])
        return calls[c]
    hand = lambda s, h, which: eng.rate_stream_handoff(s, h, which)
    _, w16p, _ = handoffs(eng, eng.new_rate_state(N, win, fs), eng.new_rate_state(N, win, fs), step, hand, range(len(calls)))
    params = tuned(w16p, w16p)
    st, plain = eng.new_rate_state(N, win, fs, alc=BASE), eng.new_rate_state(N, win, fs)
    put(st, params)
    a16, b16, w16 = handoffs(eng, st, plain, step, hand, range(len(calls)))
    want, recs, seen = expect(params, w16, delayed(a16), w16)
    assert {"speech", "silence", "limited", "unlimited"} <= seen
    assert same(b16, want) and same(st.alc, recs[:, -1]) and not same(b16, w16)


# ------------------------------------------------------------------------------------------------------- 9. capture
def test_a_captured_step_follows_the_words_and_the_gains_between_replays(eng, win):
    N = 6
    x = stepped(N, 7, 140)
    gains = {2: 6, 3: [None, 0, 6, 12, 3, 0], 4: 0, 5: [6, 6, None, None, 12, 0], 6: 20}
    params = probed(eng, win, x)
    words = {}
    for t, (i, f) in {2: (4, 4), 3: (9, 0.25), 4: (10, 0), 5: (0, 8), 6: (6, 1.5 / params[6])}.items():
        words[t] = params.copy()                                  # T x 4, c / 4, measure only, theta x 8, a_max = 1.5
        words[t][i] *= F32(f)
    p = BASE
    ref_st = eng.new_wave_state(N, win, atten_lim_db=3, ramp=True, alc=p)
    put(ref_st, params)
    ref, recs = [], []
    for t in range(7):
        if t in gains:
            ref_st.set_atten_lim_db(gains[t])
            put(ref_st, words[t])
        ref.append(eng.wave_stream_step(ref_st, x[:, 256 * t:256 * (t + 1)]).clone())
        recs.append(ref_st.alc.clone())
    assert len({bits(r).numpy().tobytes() for r in recs}) == 7 and moving(recs[-1])
    xb, yb = torch.empty(N, 256, device="cuda"), torch.empty(N, 256, device="cuda")
    st, warm = (eng.new_wave_state(N, win, atten_lim_db=3, ramp=True, alc=p) for _ in range(2))
    put(st, params)
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
            flag = st.voice()                                     # a compare on the device: capturable
    eng.wave_stream_reset(st)
    st.reset_alc()
    torch.cuda.synchronize()
    for t in range(2):                                            # the eager steps in front of the five replays
        xb.copy_(x[:, 256 * t:256 * (t + 1)])
        assert same(eng.wave_stream_step(st, xb), ref[t])
    for t in range(2, 7):
        st.set_atten_lim_db(gains[t])
        put(st, words[t])
        xb.copy_(x[:, 256 * t:256 * (t + 1)])
        g.replay()
        torch.cuda.synchronize()
        assert same(yb, ref[t]) and same(st.alc, recs[t]), t
        assert flag.tolist() == (recs[t][:, 3] != 0).tolist(), t
    assert same(st.model, ref_st.model) and same(st.wave, ref_st.wave) and same(st.gain_ramp, ref_st.gain_ramp)


# -------------------------------------------------------------------------------------------------------- 10. errors
def test_alc_with_highband_is_refused(eng, win):
    from gtcrn_micro_amd import GtcrnError
    with pytest.raises(GtcrnError):
        eng.new_rate_state(2, win, 48000, highband=0.5, alc=True)
    with pytest.raises(GtcrnError):
        eng.new_packet_state(2, win, 480, 48000, highband=0.5, alc="vad")
    with pytest.raises(GtcrnError):
        eng.new_packet_slot_state(2, win, 480, 48000, highband=0.5, alc=True)
    with pytest.raises(GtcrnError):
        eng.new_wave_state(2, win).voice()
    from gtcrn_micro_amd import alc_params
    st = eng.new_wave_state(2, win, alc=True)
    assert same(st.alc_params, alc_params())
    st.set_alc(target_dbov=-30, mode=0)
    assert same(st.alc_params, alc_params(target_dbov=-30, mode=0)) and not same(st.alc_params, alc_params())
    st.alc[:] = 7
    st.reset_alc(1, 2)
    assert same(st.alc, [[7] * 8, AK.INIT])


def test_set_alc_updates_the_states_own_configuration(eng, win):
    """set_alc replaces single settings of what alc= gave: a measure-only state stays measure-only, a mapping keeps its other
    fields, and a refused setting changes nothing."""
    from gtcrn_micro_amd import GtcrnError, alc_params
    vad = eng.new_wave_state(2, win, alc="vad")
    vad.set_alc(hang_ms=100)
    assert same(vad.alc_params, alc_params(mode=0, hang_ms=100)) and float(vad.alc_params[10]) == 0.0
    st = eng.new_wave_state(2, win, alc={"target_dbov": -20})
    st.set_alc(hang_ms=100)
    st.set_alc(ceiling_dbov=-3)
    assert same(st.alc_params, alc_params(target_dbov=-20, hang_ms=100, ceiling_dbov=-3))
    before = st.alc_params.clone()
    for bad in (dict(alpha=2), dict(treshold=1)):
        with pytest.raises(GtcrnError):
            st.set_alc(**bad)
    assert same(st.alc_params, before) and st.alc_fields["target_dbov"] == -20 and "treshold" not in st.alc_fields
    for off in (None, False):                                     # off, as meters=False and ramp=False are
        plain = eng.new_wave_state(2, win, alc=off)
        assert plain.alc is None and plain.alc_params is None
    assert eng.new_rate_state(2, win, 48000, highband=0.5, alc=False).alc is None


def test_the_c_entry_points_refuse_the_high_band_with_level_control(eng, win):
    """Python refuses alc= with highband= when the state is made; a caller of the C ABI who sets a level-control address and
    then steps a high-band form gets GTCRN_ERR_STATE, nothing is launched and the records stay."""
    from gtcrn_micro_amd import GtcrnError, alc_params
    words = torch.from_numpy(alc_params()).cuda()
    mark = torch.arange(16.0, device="cuda").reshape(2, 8) + 0.5
    states = [(eng.new_rate_state(2, win, 48000, highband=0.5), lambda s, x: eng.rate_stream_step(s, x), 768),
              (eng.new_packet_state(2, win, 480, 48000, highband=0.5), lambda s, x: eng.packet_stream_step(s, x), 480)]
    slot = eng.new_packet_slot_state(2, win, 480, 48000, highband=0.5)
    states.append((slot, lambda s, x: eng.packet_stream_step_slots(s, i32([1, 0]), x), 480))
    for st, step, n in states:
        x = stepped(2, 3, n)[:, :n].contiguous()
        for xin in (x, (x * 32767).round().to(torch.int16)):
            st.alc, st.alc_params = mark.clone(), words
            wave = st.wave.clone()
            with pytest.raises(GtcrnError, match="level control"):
                step(st, xin)
            assert same(st.alc, mark) and same(st.wave, wave)
            st.alc = st.alc_params = None
            step(st, xin)                                         # without the address the high-band step runs as before


# ----------------------------------------------------------------------------------------------------- 11. isolation
def test_a_nan_then_an_inf_in_one_stream(eng, win):
    """Stream 1 (it shares a workgroup with 0, 2 and 3) is fed a NaN, then Infs, for three hops.  Every other stream keeps
    every bit; the poisoned stream's a and S stay finite and do not move while its blocks are non-finite, and the record
    moves again once the model's history has left the poisoned frames behind."""
    N, A, B, C = 6, 4, 3, 100
    x = stepped(N, A + B + C, 150)
    xb = x.clone()
    xb[1, 256 * A + 17] = float("nan")
    xb[1, 256 * (A + 1) + 5] = float("inf")
    xb[1, 256 * (A + 2) + 200] = float("-inf")
    params = probed(eng, win, x)
    runs = []
    for inp in (x, xb):
        st = eng.new_wave_state(N, win, alc=BASE)
        put(st, params)
        o, recs, k = [], [], 0
        for h in (A, B, C):
            o.append(eng.wave_stream_step(st, inp[:, 256 * k:256 * (k + h)]))
            recs.append(npf(st.alc))
            k += h
        runs.append((torch.cat(o, 1), recs, st.wave.clone(), st.model.clone()))
    (a, ra, wa, ma), (b, rb, wb, mb) = runs
    rest = [0, 2, 3, 4, 5]
    assert same(a[rest], b[rest]) and same(wa[rest], wb[rest]) and same(ma[rest], mb[rest])
    assert all(AK.same_bits(u[rest], v[rest]) for u, v in zip(ra, rb)) and moving(ra[-1])
    assert not torch.isfinite(b[1, 256 * A:256 * (A + B)]).all() and torch.isfinite(a).all()
    assert np.isfinite(np.stack(rb)[:, 1, :2]).all()
    assert AK.same_bits(rb[1][1, :3], rb[0][1, :3])               # a, S and hang as they were
    assert rb[1][1, 3] == 0 and rb[1][1, 4] == rb[0][1, 4] and rb[1][1, 5] == rb[0][1, 5] + B
    assert rb[2][1, 5] == A + B + C - 1 and rb[2][1, 4] > rb[1][1, 4]                # voiced again
    assert not AK.same_bits(rb[2][1, :2], rb[1][1, :2]) and torch.isfinite(b[1, -256 * 8:]).all()
