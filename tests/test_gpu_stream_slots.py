"""Stream slots (gtcrn_*_slots): a call steps the resident live streams it names, in any order, and no others.  The truth is
always unchanged code -- Engine.forward_wave and the contiguous wave_stream_step / stream_step -- never another indexed call
(contract: include/gtcrn_micro_hip.h, "stream slots")."""
import numpy as np
import pytest

from conftest import load_params

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S = 23            # resident slots: the narrow form spans 6 workgroups of 4, the wide form 4 of 7, both with ragged tails
KMAX = 9          # hops of input per slot


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
    e = Engine(load_params("dns3"), 0)
    yield e
    e.stream_form(0)


@pytest.fixture(scope="module")
def win(dev):
    return torch.hann_window(512).pow(0.5).cuda()


@pytest.fixture(scope="module")
def clips(eng, win):
    """x (S, 256 KMAX) seeded * 0.1 and its offline enhancement, computed once and never modified."""
    rng = np.random.default_rng(2310)
    x = torch.from_numpy((rng.standard_normal((S, 256 * KMAX)) * 0.1).astype(np.float32)).cuda()
    ref = eng.forward_wave(x, win)
    torch.cuda.synchronize()
    return x, ref


def i32(ids):
    return torch.tensor(list(ids), dtype=torch.int32, device="cuda")


def padded(ids, n=S):
    """The call's slot table: `ids`, then the other slots (never read, but in range and distinct all the same)."""
    rest = [s for s in range(n) if s not in ids]
    return i32(list(ids) + rest)


# the ragged schedule: the slots that have a packet at each tick, in the order the server happened to gather them
ALL = list(range(S))
SCHEDULE = [
    [22, 3, 17, 0, 9, 14, 5, 20, 1, 11, 7, 19, 2, 16, 8, 21, 4, 13, 6, 18, 10, 15, 12],
    [5],
    [0, 1, 2, 3],
    [10, 4, 22, 7, 15],
    [],
    [6, 8, 9, 11, 12, 13, 14],
    [16, 17, 18, 19, 20, 21, 2, 3],
    [0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16],
    ALL,
    [21, 20, 19, 18, 17],
    [22],
    [3, 1, 2, 0],
    [12, 13, 14, 15, 16, 17, 18, 19],
    [],
    [5, 9, 22, 20, 21, 10, 11],
    list(range(8, 23)),
    [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22],
    [1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21],
    ALL[::-1],
    [7, 6],
]


def test_schedule_is_what_it_claims():
    counts = {len(t) for t in SCHEDULE}
    assert {1, 4, 5, 7, 8, 15, 23} <= counts and 0 in counts
    for s in range(S):
        active = sum(s in t for t in SCHEDULE)
        assert active >= 3 and len(SCHEDULE) - active >= 2, s
        assert active <= KMAX, s
    assert any(t != sorted(t) for t in SCHEDULE)
    assert all(len(set(t)) == len(t) and all(0 <= s < S for s in t) for t in SCHEDULE)


def run_schedule(eng, win, x, schedule=SCHEDULE):
    """Steps a fresh S-slot state through the schedule; returns (per-slot list of emitted blocks, state)."""
    st = eng.new_wave_state(S, win)
    eng.reserve(S, 1)
    seen = [0] * S
    blocks = [[] for _ in range(S)]
    xin = torch.zeros((S, 256), device="cuda")
    out = torch.empty((S, 256), device="cuda")
    for ids in schedule:
        n = len(ids)
        xin.zero_()
        for i, s in enumerate(ids):
            xin[i] = x[s, 256 * seen[s]:256 * (seen[s] + 1)]
        out.fill_(-7.0)
        eng.wave_stream_step_slots(st, padded(ids), xin, count=i32([n]), out=out)
        assert torch.equal(out[n:], torch.full_like(out[n:], -7.0)), "rows at or beyond count were written"
        for i, s in enumerate(ids):
            blocks[s].append(out[i].clone())
            seen[s] += 1
    return blocks, st


def expect(ref, s, k):
    """What slot s has emitted after k active ticks: 256 zeros, then forward_wave one hop late."""
    return torch.cat([torch.zeros(256, device="cuda"), ref[s, :256 * (k - 1)]])


@pytest.fixture(scope="module")
def ragged_runs(eng, win, clips):
    x, _ = clips
    runs = {}
    for form in (0, 2, 3):
        eng.stream_form(form)
        blocks, st = run_schedule(eng, win, x)
        runs[form] = ([torch.cat(b) for b in blocks], st.model.clone(), st.wave.clone())
    eng.stream_form(0)
    torch.cuda.synchronize()
    return runs


@pytest.mark.parametrize("form", [0, 2, 3])
def test_ragged_activity_equals_per_slot_truth(ragged_runs, clips, form):
    _, ref = clips
    got, _, _ = ragged_runs[form]
    for s in range(S):
        k = got[s].numel() // 256
        assert torch.equal(got[s], expect(ref, s, k)), (form, s)


def test_forms_give_identical_bits(ragged_runs):
    a = ragged_runs[0]
    for form in (2, 3):
        b = ragged_runs[form]
        assert all(torch.equal(p, q) for p, q in zip(a[0], b[0])), form
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), form


def test_three_launch_form_has_no_indexed_step(eng, win, clips):
    from gtcrn_micro_amd import GtcrnError
    x, _ = clips
    st = eng.new_wave_state(S, win)
    out = torch.full((4, 256), -7.0, device="cuda")
    before = (st.model.clone(), st.wave.clone())
    eng.stream_form(1)
    try:
        with pytest.raises(GtcrnError):
            eng.wave_stream_step_slots(st, i32([0, 1, 2, 3]), x[:4, :256].contiguous(), out=out)
    finally:
        eng.stream_form(0)
    assert torch.equal(out, torch.full_like(out, -7.0))
    assert torch.equal(st.model, before[0]) and torch.equal(st.wave, before[1])


@pytest.mark.parametrize("form", [2, 3])
def test_idle_slots_and_unused_rows_are_untouched(eng, win, clips, form):
    x, _ = clips
    eng.stream_form(form)
    try:
        st = eng.new_wave_state(S, win)
        eng.wave_stream_step(st, x[:, :256].contiguous())           # every slot holds history
        ids = [19, 2, 11, 7, 8]
        idle = [s for s in range(S) if s not in ids]
        m0, w0 = st.model.clone(), st.wave.clone()
        out = torch.full((S, 256), -7.0, device="cuda")
        eng.wave_stream_step_slots(st, padded(ids), x[:, 256:512].contiguous(), count=i32([len(ids)]), out=out)
        assert torch.equal(st.model[idle], m0[idle]) and torch.equal(st.wave[idle], w0[idle])
        assert not torch.equal(st.model[ids], m0[ids])
        assert torch.equal(out[len(ids):], torch.full_like(out[len(ids):], -7.0))
        m1, w1 = st.model.clone(), st.wave.clone()
        out.fill_(-7.0)
        eng.wave_stream_step_slots(st, padded(ids), x[:, 512:768].contiguous(), count=i32([0]), out=out)
        assert torch.equal(st.model, m1) and torch.equal(st.wave, w1)
        assert torch.equal(out, torch.full_like(out, -7.0))
    finally:
        eng.stream_form(0)


@pytest.mark.parametrize("limits", [None, "per_slot"])
def test_full_permutation_equals_contiguous_call(eng, win, clips, limits):
    x, _ = clips
    db = None
    if limits:
        db = [None if s % 5 == 0 else (0.0 if s % 5 == 1 else 3.0 * s) for s in range(S)]   # None-equivalent, 0 dB, distinct
    sa = eng.new_wave_state(S, win, atten_lim_db=db)
    sb = eng.new_wave_state(S, win, atten_lim_db=db)
    rng = np.random.default_rng(7)
    for k in range(8):
        p = rng.permutation(S)
        hop = x[:, 256 * k:256 * (k + 1)].contiguous()
        pt = torch.from_numpy(p).cuda()
        got = eng.wave_stream_step_slots(sa, i32(p), hop[pt].contiguous())
        want = eng.wave_stream_step(sb, hop)
        assert torch.equal(got, want[pt]), k
    assert torch.equal(sa.model, sb.model) and torch.equal(sa.wave, sb.wave)


@pytest.mark.parametrize("form", [2, 3])
def test_device_count_is_clamped_to_max_active(eng, win, clips, form):
    """slots, x and out hold M + 5 rows with valid, distinct ids; max_active = M, device count = M + 5: only M rows step.
    A missing clamp shows as a wrong answer (the five extra rows are real rows of real buffers), never as a stray access."""
    x, _ = clips
    M = 9
    ids = [14, 3, 20, 6, 9, 1, 17, 12, 5, 22, 0, 8, 19, 11]
    eng.stream_form(form)
    try:
        st = eng.new_wave_state(S, win)
        eng.wave_stream_step(st, x[:, :256].contiguous())
        m0, w0 = st.model.clone(), st.wave.clone()
        xin = x[ids, 256:512].contiguous()
        out = torch.full((M + 5, 256), -7.0, device="cuda")
        eng.wave_stream_step_slots(st, i32(ids), xin[:M], count=i32([M + 5]), out=out[:M], max_active=M)
        untouched = [s for s in range(S) if s not in ids[:M]]
        assert torch.equal(st.model[untouched], m0[untouched]) and torch.equal(st.wave[untouched], w0[untouched])
        assert torch.equal(out[M:], torch.full_like(out[M:], -7.0))
        ref = eng.new_wave_state(S, win)
        eng.wave_stream_step(ref, x[:, :256].contiguous())
        want = eng.wave_stream_step(ref, x[:, 256:512].contiguous())
        assert torch.equal(out[:M], want[ids[:M]])
    finally:
        eng.stream_form(0)


def test_join_by_reset_slots(eng, win, clips):
    x, ref = clips
    st = eng.new_wave_state(S, win)
    for k in range(3):
        eng.wave_stream_step_slots(st, i32(ALL), x[:, 256 * k:256 * (k + 1)].contiguous())
    joined = [17, 4, 21, 0, 9]
    eng.wave_stream_reset_slots(st, i32(joined))
    outs = []
    for k in range(3, 7):
        hop = x[:, 256 * k:256 * (k + 1)].clone()
        hop[joined] = x[joined, 256 * (k - 3):256 * (k - 2)]          # the new streams start their clips
        outs.append(eng.wave_stream_step_slots(st, i32(ALL), hop))
    got = torch.cat(outs, 1)
    for s in range(S):
        if s in joined:
            assert torch.equal(got[s], expect(ref, s, 4)), s
        else:
            assert torch.equal(got[s], ref[s, 256 * 2:256 * 6]), s


@pytest.mark.parametrize("r", [0, 40])
def test_leave_by_flush_slots(eng, win, r):
    rng = np.random.default_rng(40 + r)
    L = 256 * 4 + r
    x = torch.from_numpy((rng.standard_normal((S, L)) * 0.1).astype(np.float32)).cuda()
    ref = eng.forward_wave(x, win)
    st = eng.new_wave_state(S, win)
    for k in range(4):
        eng.wave_stream_step_slots(st, i32(ALL[::-1]), x[ALL[::-1], 256 * k:256 * (k + 1)].contiguous())
    leaving = [13, 2, 22, 7]
    m0, w0 = st.model.clone(), st.wave.clone()
    tail = x[leaving, 1024:].contiguous()
    last = eng.wave_stream_flush_slots(st, i32(leaving), tail)
    assert torch.equal(last, ref[leaving, -256:])
    others = [s for s in range(S) if s not in leaving]
    assert torch.equal(st.model[others], m0[others]) and torch.equal(st.wave[others], w0[others])


def test_pcm16_indexed_step(eng, win, clips):
    from gtcrn_micro_amd import f32_to_pcm16, pcm16_to_f32
    x, _ = clips
    pcm = f32_to_pcm16(x[:, :256 * 4].contiguous())
    sa, sb = eng.new_wave_state(S, win), eng.new_wave_state(S, win)
    ids = [20, 1, 15, 8, 3, 11]
    for k in range(4):
        hop = pcm[ids, 256 * k:256 * (k + 1)].contiguous()
        got = eng.wave_stream_step_slots(sa, i32(ids), hop)
        want = f32_to_pcm16(eng.wave_stream_step_slots(sb, i32(ids), pcm16_to_f32(hop)))
        assert got.dtype == torch.int16 and torch.equal(got, want), k


@pytest.mark.parametrize("form", [2, 3])
def test_spec_level_step_slots(eng, form):
    rng = np.random.default_rng(11)
    spec = torch.from_numpy((rng.standard_normal((3, 257, 4, 2)) * 0.1).astype(np.float32)).cuda()
    ids = [7, 2, 5]
    eng.stream_form(form)
    try:
        st = eng.new_state(9)
        m0 = st.clone()
        singles = [eng.new_state(1) for _ in ids]
        for t in range(4):
            frame = spec[:, :, t:t + 1].contiguous()
            got = eng.stream_step_slots(st, i32(ids), frame)
            for i in range(3):
                assert torch.equal(got[i:i + 1], eng.stream_step(singles[i], frame[i:i + 1])), (t, i)
        for i, s in enumerate(ids):
            assert torch.equal(st[s:s + 1], singles[i])
        idle = [s for s in range(9) if s not in ids]
        assert torch.equal(st[idle], m0[idle])
    finally:
        eng.stream_form(0)


def test_graph_replay_serves_a_changing_active_set(eng, win, clips):
    x, _ = clips
    M = 13
    rng = np.random.default_rng(5)
    ticks = []
    for k, n in enumerate([13, 0, 5, 13, 1, 7, 4, 0, 12, 8, 13, 3]):
        ticks.append((rng.permutation(S)[:M], n))
    seen = [0] * S

    def rows(perm, n):
        xin = torch.zeros((M, 256), device="cuda")
        for i in range(n):
            s = int(perm[i])
            xin[i] = x[s, 256 * (seen[s] % KMAX):256 * (seen[s] % KMAX + 1)]
        return xin

    inputs = []
    for perm, n in ticks:
        inputs.append(rows(perm, n))
        for i in range(n):
            seen[int(perm[i])] += 1
    # eager
    se = eng.new_wave_state(S, win)
    eager = [eng.wave_stream_step_slots(se, i32(p), xin, count=i32([n])).clone()[:n] for (p, n), xin in zip(ticks, inputs)]
    # one capture, twelve replays
    sg = eng.new_wave_state(S, win)
    eng.reserve(M, 1)
    slots, count = i32(ticks[0][0]), i32([0])
    xin, out = torch.zeros((M, 256), device="cuda"), torch.zeros((M, 256), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.wave_stream_step_slots(sg, slots, xin, count=count, out=out)     # warm-up with count 0: nothing steps
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.wave_stream_step_slots(sg, slots, xin, count=count, out=out)
    for k, ((p, n), xk) in enumerate(zip(ticks, inputs)):
        slots.copy_(i32(p))
        count.fill_(n)
        xin.copy_(xk)
        graph.replay()
        assert torch.equal(out[:n], eager[k]), k
    assert torch.equal(sg.model, se.model) and torch.equal(sg.wave, se.wave)


def test_bad_arguments_and_check_slots(eng, win, clips):
    from gtcrn_micro_amd import GtcrnError
    x, _ = clips
    st = eng.new_wave_state(S, win)
    hop = x[:4, :256].contiguous()
    out = torch.full((4, 256), -7.0, device="cuda")
    good = i32([3, 9, 1, 20])
    bad_calls = [
        lambda: eng.wave_stream_step_slots(st, good.long(), hop, out=out),                       # dtype
        lambda: eng.wave_stream_step_slots(st, good.cpu(), hop, out=out),                        # device
        lambda: eng.wave_stream_step_slots(st, good, x[:4, :512].contiguous(), out=out),         # two hops
        lambda: eng.wave_stream_step_slots(st, good, x[:5, :256].contiguous(), out=out),         # rows != max_active
        lambda: eng.wave_stream_step_slots(st, good, hop, count=torch.tensor([4]).cuda(), out=out),   # int64 count
        lambda: eng.wave_stream_step_slots(eng.new_rate_state(S, win, 48000), good, hop, out=out),
        lambda: eng.wave_stream_step_slots(eng.new_packet_state(S, win, 160), good, hop, out=out),
    ]
    before = (st.model.clone(), st.wave.clone())
    for i, c in enumerate(bad_calls):
        with pytest.raises(GtcrnError):
            c()
        assert torch.equal(out, torch.full_like(out, -7.0)), i
    assert torch.equal(st.model, before[0]) and torch.equal(st.wave, before[1])
    # the synchronous validator works on the host copy; such a list never reaches a kernel
    assert eng.check_slots(st, good) == 4
    with pytest.raises(GtcrnError):
        eng.check_slots(st, i32([3, 9, 3, 20]))
    with pytest.raises(GtcrnError):
        eng.check_slots(st, i32([3, 9, S, 20]))
    assert eng.check_slots(st, i32([3, 9, 3, 20]), count=i32([2])) == 2      # the repeated id is beyond count


def test_streaming_wrapper_passes_slots_through(win, clips):
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd.streaming.gtcrn_micro_stream import StreamGTCRNMicro
    x, _ = clips
    stream = StreamGTCRNMicro().cuda().eval()
    rows = [5, 18, 2]
    ids = i32(rows)
    st, truth = stream.init_wave_state(S, win), stream.init_wave_state(S, win)
    for k in range(3):
        hop = x[:, 256 * k:256 * (k + 1)].contiguous()
        assert torch.equal(stream.step_wave(hop[rows].contiguous(), st, slots=ids), stream.step_wave(hop, truth)[rows]), k
    # a stream joins at slot 18; the others go on
    assert stream.init_wave_state(S, win, state=st, slots=i32([18])) is st
    stream.engine(x.device).wave_stream_reset(truth, 18, 19)
    hop = x[:, 768:1024].contiguous()
    assert torch.equal(stream.step_wave(hop[rows].contiguous(), st, slots=ids), stream.step_wave(hop, truth)[rows])
    tail = x[:, 1024:1064].contiguous()
    assert torch.equal(stream.flush_wave(tail[rows].contiguous(), st, slots=ids), stream.flush_wave(tail, truth)[rows])
    with pytest.raises(GtcrnError):
        stream.step_wave(x[:3, :256].contiguous(), stream.init_wave_state(S, win, fs=48000), slots=ids)
    with pytest.raises(GtcrnError):
        stream.step_wave(x[:3, :160].contiguous(), stream.init_wave_state(S, win, packet=160), slots=ids)
