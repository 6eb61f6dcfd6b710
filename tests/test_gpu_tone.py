"""The tone guard (include/gtcrn_micro_hip.h, "tone guard") on every live waveform path.  The checker (tests/tone_checker.py)
is the contract in numpy float32; a twin state WITHOUT tones, fed the same input, supplies the wet blocks w, because its
outputs are what the other test files pin.  Of every three streams one carries noise plus an 80 ms digit that starts
mid-block, one a 2100 Hz tone and one noise only; every test asserts from the checker's trace (or from the records) that
guarded, held, unguarded and reported blocks all occurred.  Every comparison is exact.

Every test here that makes a state with tones= fails on a library without the tone guard (GtcrnError at the constructor);
only test_the_c_entry_point_checks_its_arguments's Python half and the helpers run there."""
import numpy as np
import pytest

from conftest import load_params
import alc_checker as AK
import tone_checker as TK

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
TAB = TK.table()
HOPS = [1, 2, 3, 1, 1, 2, 3, 2, 1, 3]                         # 10 calls, 19 blocks
MIXED = {"zero", "passed_dry", "guard_candidate", "guard_hold", "unguarded", "reported", "candidate_waits"}
ALC = dict(hang_ms=32, ratio_db=-60, rise_db_s=300, fall_db_s=600, target_dbov=-20, min_gain_db=-12, max_gain_db=30)


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


def same(a, b):
    a, b = (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, np.float32)) for v in (a, b))
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def signal(N, n, seed, fs=16000):
    """(N, n) float32 at fs: stream s carries, by s % 3, noise plus an 80 ms digit that starts 4.4 blocks in; faint noise plus
    a 2100 Hz tone from 3.2 blocks in for 9 blocks; noise only."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = np.empty((N, n))
    for s in range(N):
        if s % 3 == 0:
            r, c = divmod((5 + s) % 16, 4)
            on = (t >= 4.4 * 0.016) & (t < 4.4 * 0.016 + 0.080)
            x[s] = 0.01 * rng.standard_normal(n) + on * 0.1 * (np.sin(2 * np.pi * TK.FREQS[r] * t) + np.sin(2 * np.pi * TK.FREQS[4 + c] * t))
        elif s % 3 == 1:
            on = (t >= 3.2 * 0.016) & (t < 12.2 * 0.016)
            x[s] = 0.002 * rng.standard_normal(n) + on * 0.2 * np.sin(2 * np.pi * 2100 * t)
        else:
            x[s] = 0.05 * rng.standard_normal(n)
    return torch.from_numpy(x.astype(np.float32)).cuda()


def delayed(x):
    """The dry samples under the blocks of a stream stepped from its reset: the input one hop late."""
    return np.concatenate([np.zeros_like(x[:, :256]), x[:, :-256]], 1)


def blocks(a):
    a = np.asarray(a, np.float32)
    return a.reshape(a.shape[0], -1, 256)


def expect(params, w, x, first=0, rec0=None, gain=None, ramp_word=None, **kw):
    """The checker for N streams: w, x (N, 256 K) numpy -> a dict of y (N, 256 K), records (N, K, 8), ramp (N, K), alc
    (N, K, 8), meters (N, K, 4) and the union of the traces."""
    runs = [TK.stream(params, TAB, blocks(w)[s], blocks(x)[s], first_block_index=first, record=None if rec0 is None else rec0[s],
                      gain=None if gain is None else gain[s], ramp_word=None if ramp_word is None else ramp_word[s], **kw)
            for s in range(len(w))]
    out = {k: np.stack([np.asarray(r[k], np.float32) for r in runs]) for k in ("y", "records", "alc", "m")}
    out["y"] = out["y"].reshape(len(w), -1)
    out["ramp"] = [r["ramp"] for r in runs]
    out["meters"] = [r["meters"] for r in runs]
    out["traces"] = [r["traces"] for r in runs]
    out["seen"] = TK.seen(t for r in runs for t in [TK.seen(r["traces"])])
    return out


def run_hops(eng, st, x, hops, each=None):
    outs, k = [], 0
    for c, h in enumerate(hops):
        if each is not None:
            each(c, k)
        outs.append(eng.wave_stream_step(st, x[:, 256 * k:256 * (k + h)]))
        k += h
    return torch.cat(outs, 1)


def occurred(rec):
    """From final records alone: some stream reported a tone and guarded some, not all, of its blocks."""
    rec = npf(rec)
    return (rec[:, 5] > 0).any() and 0 < rec[:, 6].sum() < rec[:, 7].sum()


# ------------------------------------------------------------------------------------------------------ 1. hop form
@pytest.mark.parametrize("N", [1, 3, 6])
@pytest.mark.parametrize("pcm", [False, True])
def test_hop_form_equals_the_checker(eng, win, N, pcm):
    """Outputs, the records after every call, state.tone() and both state tensors, without gains; a guarded block is the dry
    input one hop late."""
    from gtcrn_micro_amd import pcm16_to_f32, f32_to_pcm16, tone_params
    K = sum(HOPS)
    xf = signal(N, 256 * K, 10 + N)
    if pcm:
        x16 = (xf * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        xf = pcm16_to_f32(x16.contiguous())
    xin = x16 if pcm else xf
    plain, plain_in = eng.new_wave_state(N, win), eng.new_wave_state(N, win)
    w = npf(run_hops(eng, plain, xf, HOPS))
    run_hops(eng, plain_in, xin, HOPS)
    st = eng.new_wave_state(N, win, tones=True)
    assert tuple(st.tones.shape) == (N, 8) and tuple(st.tone_params.shape) == (16,) and not st.tones.any()
    assert same(st.tone_params, TK.params()) and same(st.tone_table, TAB) and same(st.tone_params, tone_params())
    want = expect(TK.params(), w, delayed(npf(xf)))
    need = MIXED - (set() if N > 1 else {"candidate_waits"})
    assert need <= want["seen"], sorted(need - want["seen"])
    recs, done = want["records"], []

    def after_previous(c, k):
        if k:
            assert same(st.tones, recs[:, k - 1]), c
            assert st.tone().dtype == torch.int32 and st.tone().tolist() == recs[:, k - 1, 0].astype(int).tolist(), c
        done.append(k)

    got = run_hops(eng, st, xin, HOPS, after_previous)
    assert same(st.tones, recs[:, -1]) and len(done) == len(HOPS)
    assert st.tone_events().tolist() == recs[:, -1, 5].astype(int).tolist()
    y = torch.from_numpy(want["y"]).cuda()
    assert torch.equal(got, f32_to_pcm16(y.contiguous())) if pcm else same(got, y)
    assert torch.equal(st.wave, plain_in.wave) and torch.equal(st.model, plain_in.model)
    guarded = 0
    for s in range(N):
        for k in range(1, K):
            if "passed_dry" in want["traces"][s][k]:
                assert torch.equal(got[s, 256 * k:256 * (k + 1)], xin[s, 256 * (k - 1):256 * k]), (s, k)
                guarded += 1
    assert guarded >= 5
    assert not torch.equal(got, run_hops(eng, eng.new_wave_state(N, win), xin, HOPS))


# ------------------------------------------------------------------------------------------------- 2. detect only
@pytest.mark.parametrize("kw", [dict(), dict(atten_lim_db=[6, None, 0, 12, 3, 6]), dict(meters=True),
                                dict(atten_lim_db=[6, None, 0, 12, 3, 6], ramp=True), dict(alc=ALC, meters=True)],
                         ids=["plain", "limit", "meters", "limit+ramp", "alc+meters"])
def test_detect_mode_leaves_every_bit_alone(eng, win, kw):
    N, K = 6, sum(HOPS)
    x = signal(N, 256 * K, 20)
    st, twin = eng.new_wave_state(N, win, tones="detect", **kw), eng.new_wave_state(N, win, **kw)
    assert float(st.tone_params[9]) == 0.0
    moves = lambda s: (lambda c, k: s.set_atten_lim_db(12 if c % 2 else [0, 6, None, 3, 12, 6])) if "atten_lim_db" in kw else None
    m = run_hops(eng, twin, x, HOPS, moves(twin))
    got = run_hops(eng, st, x, HOPS, moves(st))
    assert same(got, m) and same(st.wave, twin.wave) and same(st.model, twin.model)
    if kw.get("meters"):
        assert same(st.meters, twin.meters)
    if kw.get("ramp"):
        assert same(st.gain_ramp, twin.gain_ramp)
    if kw.get("alc"):
        assert same(st.alc, twin.alc) and (npf(st.alc)[:, 4] > 0).any()
    recs, traces = zip(*[TK.detect(TK.params(mode=0), TAB, npf(x)[s, :-256]) for s in range(N)])
    assert same(st.tones, np.stack([r[-1] for r in recs])) and occurred(st.tones)
    assert {"guard_candidate", "guard_hold", "unguarded", "reported"} <= TK.seen(t for tr in traces for t in tr)


# ------------------------------------------------------------------------------ 3. gains, ramps, meters and level control
def test_guard_with_gains_ramps_meters_and_level_control(eng, win):
    """A guarded block snaps to dry gain 1 and the block behind the hold ramps 1 -> g; level control and the meters see m."""
    from gtcrn_micro_amd import alc_params
    N, K = 6, sum(HOPS)
    x = signal(N, 256 * K, 30)
    lim = [6, 12, 3, 20, 6, 12]
    w = npf(run_hops(eng, eng.new_wave_state(N, win), x, HOPS))
    ap = alc_params(**ALC)
    ap[0] = F32(np.median([AK.hop_sum(b) for s in blocks(w)[:, 1:] for b in s]))
    st = eng.new_wave_state(N, win, atten_lim_db=lim, ramp=True, meters=True, alc=ALC, tones=True)
    st.alc_params.copy_(torch.from_numpy(ap))
    g = npf(st.dry_gain)
    got = run_hops(eng, st, x, HOPS)
    want = expect(TK.params(), w, delayed(npf(x)), gain=g, ramp_word=g, alc_params=ap, meters=np.zeros(4, np.float32))
    assert MIXED | {"ramps_from_1", "alc_speech", "alc_silence"} <= want["seen"], sorted(want["seen"])
    assert same(got, want["y"]) and same(st.tones, want["records"][:, -1]) and same(st.alc, want["alc"][:, -1])
    assert same(st.gain_ramp, np.asarray([r[-1] for r in want["ramp"]], np.float32))
    assert same(st.meters, np.stack([m[-1] for m in want["meters"]]))
    assert not same(want["y"], want["m"].reshape(N, -1))         # the level control moved the output ...
    k = [k for k in range(K) if "passed_dry" in want["traces"][1][k]][0]
    assert same(want["m"][1, k], npf(x)[1, 256 * (k - 1):256 * k])      # ... of blocks that hold the dry signal


# ------------------------------------------------------------------------------------------- 4. hop cuts, flush, join
@pytest.mark.parametrize("r", [0, 100])
def test_the_cut_of_hops_does_not_matter_and_the_flush_block_is_a_block(eng, win, r):
    N = 3
    x = signal(N, 256 * 12, 40)[:, 256 * 3:256 * 9 + r].contiguous()      # (the tone and the digit are on from the start)
    plain = eng.new_wave_state(N, win)
    w = npf(torch.cat([eng.wave_stream_step(plain, x[:, :1536]), eng.wave_stream_flush(plain, x[:, 1536:])], 1))
    lim = [6, 12, 3]
    runs = []
    for cut in ([4], [1, 1, 1, 1], [2, 2]):
        st = eng.new_wave_state(N, win, tones=True, atten_lim_db=lim, ramp=True)
        o = [eng.wave_stream_step(st, x[:, :512])]
        o.append(run_hops(eng, st, x[:, 512:1536], cut))
        o.append(eng.wave_stream_flush(st, x[:, 1536:]))
        assert same(st.wave, plain.wave) and same(st.model, plain.model)
        runs.append((torch.cat(o, 1), st.tones.clone(), st.gain_ramp.clone()))
    for other in runs[1:]:
        assert all(same(a, b) for a, b in zip(runs[0], other))
    dry = np.concatenate([delayed(npf(x[:, :1536])), npf(x[:, 1280:1536])], 1)       # the flush block lies over the ring's newest hop
    g = npf(st.dry_gain)
    want = expect(TK.params(), w, dry, gain=g, ramp_word=g)
    assert {"passed_dry", "unguarded", "reported"} <= want["seen"]
    assert same(runs[0][0], want["y"]) and same(runs[0][1], want["records"][:, -1]) and (want["records"][:, -1, 7] == 6).all()


def test_a_flush_without_a_block_leaves_the_record_alone(eng, win):
    N = 3
    x = signal(N, 256, 41) + 0.5
    st = eng.new_wave_state(N, win, tones=True)
    mark = torch.arange(8.0 * N, device="cuda").reshape(N, 8) + 0.5
    st.tones.copy_(mark)
    assert not eng.wave_stream_step(st, x).any() and not st.tones.any()      # the structural zero: eight zeros
    st.tones.copy_(mark)
    assert not eng.wave_stream_flush(st, x[:, :0]).any() and same(st.tones, mark)      # 256 samples in all: no block
    st2 = eng.new_wave_state(N, win, tones=True)
    st2.tones.copy_(mark)
    assert not eng.wave_stream_flush(st2, x[:, :200]).any() and same(st2.tones, mark)


def test_a_join_resets_only_the_named_record(eng, win):
    N = 3
    x = signal(N, 256 * 12, 42)
    a, b = eng.new_wave_state(N, win, tones=True), eng.new_wave_state(N, win)
    o = [eng.wave_stream_step(a, x[:, :256 * 9])]
    wb = [eng.wave_stream_step(b, x[:, :256 * 9])]
    rec9 = npf(a.tones)
    assert rec9[1, 4] == 1 and rec9[1, 0] == 18                   # stream 1 joins while its tone is guarded
    for s in (a, b):
        eng.wave_stream_reset_slots(s, i32([1]))
    o.append(eng.wave_stream_step(a, x[:, 256 * 9:]))
    wb.append(eng.wave_stream_step(b, x[:, 256 * 9:]))
    w, xn = npf(torch.cat(wb, 1)), npf(x)
    first = expect(TK.params(), w[:, :256 * 9], delayed(xn[:, :256 * 9]))
    assert same(o[0], first["y"]) and same(rec9, first["records"][:, -1])
    dry2 = xn[:, 256 * 8:-256]
    rest = [0, 2]
    cont = expect(TK.params(), w[rest, 256 * 9:], dry2[rest], first=9, rec0=rec9[rest])
    assert same(o[1][rest], cont["y"]) and same(a.tones[rest], cont["records"][:, -1])
    fresh = expect(TK.params(), w[1:2, 256 * 9:], dry2[1:2], first=0)
    assert "zero" in fresh["seen"] and same(o[1][1:2], fresh["y"]) and same(a.tones[1:2], fresh["records"][:, -1])
    assert fresh["records"][0, -1, 7] == 2 and cont["records"][0, -1, 7] == 11


# --------------------------------------------------------------------------------------------------------- 5. slots
def test_slots_step_the_named_and_leave_the_rest_alone(eng, win):
    """Six resident streams; after two contiguous hops the calls name slots 4, 0, 3 and, beyond the device count of 3, slot
    5.  The named slots equal the contiguous form of the same streams, the others keep every bit."""
    S, K = 6, 12
    x = signal(S, 256 * K, 50)
    w = npf(eng.wave_stream_step(eng.new_wave_state(S, win), x))
    want = expect(TK.params(), w, delayed(npf(x)))
    st = eng.new_wave_state(S, win, tones=True)
    eng.wave_stream_step(st, x[:, :512])
    table, cnt, named = i32([4, 0, 3, 5]), i32([3]), [4, 0, 3]
    rest = [1, 2, 5]
    st.tones[rest] += 0.25                                       # marks: an idle slot's record is neither read nor written
    before = [t.clone() for t in (st.tones, st.wave, st.model)]
    y = torch.from_numpy(want["y"]).cuda()
    for k in range(2, K):
        rows = x[[4, 0, 3, 5], 256 * k:256 * (k + 1)].contiguous()
        out = torch.full_like(rows, 77)
        eng.wave_stream_step_slots(st, table, rows, count=cnt, out=out)
        assert (out[3] == 77).all()                               # beyond the count: not written
        assert same(out[:3], y[named, 256 * k:256 * (k + 1)].contiguous()), k
        assert same(st.tones[named], want["records"][named, k]), k
        for t, b in zip((st.tones, st.wave, st.model), before):
            assert same(t[rest], b[rest]), k
    assert occurred(st.tones[named])


# -------------------------------------------------------------------------------------------------- 6. packet forms
def test_packet_group_at_16k_equals_the_hop_form(eng, win):
    """The 16 kHz hand-off is the hop stream: a hop-form state with tones, fed the inbound hand-off, emits the outbound one
    and ends every call with the same records."""
    N, C, n = 3, 28, 160
    x = signal(N, n * C, 60)
    st, hop = eng.new_packet_state(N, win, n, 16000, tones=True), eng.new_wave_state(N, win, tones=True)
    hops = 0
    for c in range(C):
        h = st.next_hops
        before = st.tones.clone()
        eng.packet_stream_step(st, x[:, n * c:n * (c + 1)].contiguous())
        if h == 0:
            assert same(st.tones, before), c                      # no hop: the records stay
            continue
        a16, b16 = eng.packet_stream_handoff(st, 0), eng.packet_stream_handoff(st, 1)
        assert same(eng.wave_stream_step(hop, a16), b16) and same(st.tones, hop.tones), c
        hops += h
    assert hops >= 16 and occurred(st.tones) and same(st.wave, hop.wave)


def test_packet_slots_equal_one_stream_groups(eng, win):
    """Three resident slots on a ragged schedule (so their phases differ); every slot is the one-stream group fed the same
    packets, outputs and records."""
    S, T, n, fs = 3, 20, 320, 16000
    rng = np.random.default_rng(61)
    st = eng.new_packet_slot_state(S, win, n, fs, tones=True)
    singles = [eng.new_packet_state(1, win, n, fs, tones=True) for _ in range(S)]
    x = signal(S, n * T, 62)
    fed = [0] * S
    phases = set()
    for t in range(T):
        act = [int(s) for s in rng.permutation(S) if rng.random() < 0.75] or [int(rng.integers(S))]
        if t == 0:
            act = [int(s) for s in rng.permutation(S)]
        xin = torch.stack([x[s, n * fed[s]:n * (fed[s] + 1)] for s in act])
        got = eng.packet_stream_step_slots(st, i32(act), xin)
        for i, s in enumerate(act):
            assert same(got[i:i + 1], eng.packet_stream_step(singles[s], xin[i:i + 1])), (t, s)
            fed[s] += 1
        assert same(st.tones, torch.cat([u.tones for u in singles])), t
        phases.add(tuple(st.phase.tolist()))
    assert any(len(set(q)) > 1 for q in phases) and len(set(fed)) > 1 and occurred(st.tones)


# ------------------------------------------------------------------------------------- 7. G.711 and the rate form
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
    codes = f32_to_g711(signal(N, n * C, 70, fs).contiguous(), "ulaw")
    xf = g711_to_f32(codes.contiguous(), "ulaw")

    def step(s, c, feed=lambda t: t):
        h = s.next_hops
        s.out.append(eng.packet_stream_step(s, feed(xf[:, n * c:n * (c + 1)].contiguous())))
        return h
    hand = lambda s, h, which: eng.packet_stream_handoff(s, which)
    runs = {}
    for law in (None, "ulaw"):
        st, tw = eng.new_packet_state(N, win, n, fs, tones=True, g711=law), eng.new_packet_state(N, win, n, fs)
        st.out, tw.out = [], []
        feed = (lambda t: f32_to_g711(t, "ulaw")) if law else (lambda t: t)
        stp = lambda s, c: step(s, c, feed if s is st else (lambda t: t))
        a16, b16, w16 = handoffs(eng, st, tw, stp, hand, range(C))
        runs[law] = (a16, b16, torch.cat(st.out, 1), st.tones.clone())
        want = expect(TK.params(), w16, delayed(a16))
        assert {"passed_dry", "guard_hold", "unguarded", "reported"} <= want["seen"], sorted(want["seen"])
        assert same(b16, want["y"]) and same(st.tones, want["records"][:, -1]), law
    assert runs["ulaw"][2].dtype == torch.uint8 and same(runs["ulaw"][1], runs[None][1]) and same(runs["ulaw"][3], runs[None][3])
    assert torch.equal(runs["ulaw"][2], f32_to_g711(runs[None][2].contiguous(), "ulaw"))


def test_rate_form_through_its_16k_handoff(eng, win):
    fs, H, N = 48000, 768, 3
    calls = [1, 2, 1, 3, 2, 3, 2, 2]
    x = signal(N, H * sum(calls), 71, fs)
    offs = np.concatenate([[0], np.cumsum(calls)])

    def step(s, c):
        eng.rate_stream_step(s, x[:, H * offs[c]:H * offs[c + 1]])
        return calls[c]
    hand = lambda s, h, which: eng.rate_stream_handoff(s, h, which)
    st, plain = eng.new_rate_state(N, win, fs, tones=True), eng.new_rate_state(N, win, fs)
    a16, b16, w16 = handoffs(eng, st, plain, step, hand, range(len(calls)))
    want = expect(TK.params(), w16, delayed(a16))
    assert {"passed_dry", "guard_hold", "unguarded", "reported"} <= want["seen"], sorted(want["seen"])
    assert same(b16, want["y"]) and same(st.tones, want["records"][:, -1]) and not same(b16, w16)


def test_high_band_with_gains_returns_the_input_under_a_guarded_block(eng, win):
    """highband = 1 at 48 kHz with a limit: under guarded blocks beta = 1 and gamma = 1, the bypass identity -- the output is the
    input at the form's latency, bit for bit, wherever the outbound filter sees guarded blocks only."""
    fs, H, N, K = 48000, 768, 3, 16
    x = signal(N, H * K, 72, fs)
    st = eng.new_rate_state(N, win, fs, atten_lim_db=12, highband=1.0, tones=True)
    twin = eng.new_rate_state(N, win, fs, atten_lim_db=12, highband=1.0)
    y, recs = [], []
    for k in range(K):
        y.append(eng.rate_stream_step(st, x[:, H * k:H * (k + 1)]).clone())
        recs.append(npf(st.tones))
    y, guard = torch.cat(y, 1), np.stack(recs)[:, :, 4]          # (K, N): block k of every stream guarded?
    t = torch.cat([eng.rate_stream_step(twin, x[:, H * k:H * (k + 1)]).clone() for k in range(K)], 1)
    lat, inside, outside = st.latency, 0, 0
    for s in range(N):
        for k in range(3, K):
            sl = slice(H * k, H * (k + 1))
            if guard[k - 2:k + 1, s].all():
                assert torch.equal(y[s, sl], x[s, H * k - lat:H * (k + 1) - lat]), (s, k)
                assert not torch.equal(t[s, sl], y[s, sl])
                inside += 1
            elif not guard[k - 3:k + 1, s].any():
                assert torch.equal(y[s, sl], t[s, sl]), (s, k)     # no guard in reach: the call without tones
                outside += 1
    assert inside >= 3 and outside >= 3


# ------------------------------------------------------------------------------------------------------- 8. capture
def test_a_captured_step_follows_rewritten_parameter_words(eng, win):
    N, K = 3, 12
    x = signal(N, 256 * K, 80)
    mode = {k: int(k < 7 or k >= 10) for k in range(K)}           # guard, detect only from block 7, guard again from 10
    ref_st = eng.new_wave_state(N, win, atten_lim_db=6, ramp=True, tones=True)
    ref, recs = [], []
    for k in range(K):
        ref_st.set_tones(mode=mode[k])
        ref.append(eng.wave_stream_step(ref_st, x[:, 256 * k:256 * (k + 1)]).clone())
        recs.append(ref_st.tones.clone())
    plain = run_hops(eng, eng.new_wave_state(N, win, atten_lim_db=6, ramp=True), x, [1] * K)
    diff = [k for k in range(K) if not same(ref[k], plain[:, 256 * k:256 * (k + 1)])]
    assert diff and 8 not in diff and 9 not in diff and min(diff) < 7 and max(diff) >= 10      # (7 ramps back from 1)
    xb, yb = torch.empty(N, 256, device="cuda"), torch.empty(N, 256, device="cuda")
    st, warm = (eng.new_wave_state(N, win, atten_lim_db=6, ramp=True, tones=True) for _ in range(2))
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
            code = st.tone()                                      # a conversion on the device: capturable
    eng.wave_stream_reset(st)
    st.reset_tones()
    st.gain_ramp.copy_(st.dry_gain)
    torch.cuda.synchronize()
    for k in range(2):                                            # the eager steps in front of the replays
        xb.copy_(x[:, 256 * k:256 * (k + 1)])
        assert same(eng.wave_stream_step(st, xb), ref[k])
    for k in range(2, K):
        st.set_tones(mode=mode[k])
        xb.copy_(x[:, 256 * k:256 * (k + 1)])
        g.replay()
        torch.cuda.synchronize()
        assert same(yb, ref[k]) and same(st.tones, recs[k]), k
        assert code.tolist() == npf(recs[k])[:, 0].astype(int).tolist(), k
    assert same(st.model, ref_st.model) and same(st.wave, ref_st.wave) and same(st.gain_ramp, ref_st.gain_ramp)
    assert occurred(st.tones)


# ------------------------------------------------------------------------------------------------------ 9. isolation
def test_a_nan_then_infs_in_one_stream(eng, win):
    """Stream 2 (it shares a workgroup with 0, 1 and 3) is fed a NaN, then Infs, for three hops.  Every other stream keeps
    every bit of its output, states and record; the poisoned stream has no candidate in those blocks and a finite record."""
    N, A, B, C = 6, 4, 3, 5
    x = signal(N, 256 * (A + B + C), 90)
    xb = x.clone()
    xb[2, 256 * A + 17] = float("nan")
    xb[2, 256 * (A + 1) + 5] = float("inf")
    xb[2, 256 * (A + 2) + 200] = float("-inf")
    runs = []
    for inp in (x, xb):
        st = eng.new_wave_state(N, win, tones=True)
        o, recs, k = [], [], 0
        for h in (A, B, 1, C - 1):
            o.append(eng.wave_stream_step(st, inp[:, 256 * k:256 * (k + h)]))
            recs.append(npf(st.tones))
            k += h
        runs.append((torch.cat(o, 1), recs, st.wave.clone(), st.model.clone()))
    (a, ra, wa, ma), (b, rb, wb, mb) = runs
    rest = [0, 1, 3, 4, 5]
    assert same(a[rest], b[rest]) and same(wa[rest], wb[rest]) and same(ma[rest], mb[rest])
    assert all(TK.same_bits(u[rest], v[rest]) for u, v in zip(ra, rb)) and occurred(ra[-1])
    assert np.isfinite(np.stack(rb)).all()
    assert rb[2][2, 1] == 0 and rb[2][2, 2] == 0 and rb[2][2, 7] == A + B       # the last poisoned block: no candidate
    assert rb[-1][2, 7] == A + B + C - 1


# -------------------------------------------------------------------------------------------------------- 10. errors
def test_the_c_entry_point_checks_its_arguments(eng, win):
    from gtcrn_micro_amd import GtcrnError, _lib, tone_params
    L = _lib.lib()
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    assert p % 32 == 0
    fn = L.gtcrn_wave_stream_set_tone
    for args in ((None, p, p, p), (eng._h, p, None, None), (eng._h, p, p, None), (eng._h, None, p, p), (eng._h, None, None, p),
                 (eng._h, p + 16, p, p), (eng._h, p, p + 8, p), (eng._h, p, p, p + 4)):
        assert fn(*args) == -1, args
    assert fn(eng._h, p, p + 16, p + 16) == 0 and fn(eng._h, None, None, None) == 0
    with pytest.raises(GtcrnError):
        eng.new_wave_state(2, win).tone()
    with pytest.raises(GtcrnError):
        eng.new_wave_state(2, win, tones="on")
    st = eng.new_wave_state(2, win, tones="detect")
    st.set_tones(hold_blocks=3)
    assert same(st.tone_params, tone_params(mode=0, hold_blocks=3))
    before = st.tone_params.clone()
    for bad in (dict(pair_purity=2), dict(hold=1)):
        with pytest.raises(GtcrnError):
            st.set_tones(**bad)
    assert same(st.tone_params, before)
    st.tones[:] = 7
    st.reset_tones(1, 2)
    assert same(st.tones, [[7] * 8, [0] * 8])
    for off in (None, False):
        assert eng.new_wave_state(2, win, tones=off).tones is None
    # tones and the high band go together; level control with the high band is refused as before
    assert eng.new_rate_state(2, win, 48000, highband=0.5, tones=True).tones is not None
    with pytest.raises(GtcrnError):
        eng.new_rate_state(2, win, 48000, highband=0.5, tones=True, alc=True)
