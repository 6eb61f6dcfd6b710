"""The conference mix on the device (include/gtcrn_micro_hip.h, "conference rooms"): the kernel against the
contract in numpy float32 (tests/mixer_checker.py), bit for bit, over the cases the host twin runs (tests/mixer_cases.py), in
float and int16; then the Mixer class, captured calls whose tables, parameters and room count are rewritten between replays,
and the bridge end to end behind a packet-slot state."""
import numpy as np
import pytest
import torch

from conftest import load_params
import mixer_checker as MK
import mixer_cases as MC

pytestmark = pytest.mark.gpu
F = np.float32
CASES = MC.all_cases()
POISON = MC.poison_cases()


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


def whole(v):
    """The buffer a row view was cut from."""
    return v if v.base is None else v.base


def kernel(x, out, room_start, seats, rec, params, nrooms, voice):
    """The raw entry on device copies of the very buffers (row pitch included); out and rec are copied back in place."""
    from gtcrn_micro_amd import _lib
    n, item = x.shape[1], x.dtype.itemsize
    xb, ob = torch.from_numpy(whole(x).copy()).cuda(), torch.from_numpy(whole(out).copy()).cuda()
    st = i32(room_start)
    se = i32(np.concatenate([np.asarray(seats, np.int32).reshape(-1), np.zeros(4, np.int32)]))
    rc, pr = torch.from_numpy(rec.copy()).cuda(), torch.from_numpy(np.asarray(params, F)).cuda()
    nr = None if nrooms is None else i32([nrooms])
    vb, vptr, vstride = None, None, 0
    if voice is not None:
        vb = torch.from_numpy(whole(voice).copy()).cuda()
        vptr, vstride = vb.data_ptr() + voice.ctypes.data - whole(voice).ctypes.data, voice.strides[0] // 4
    fn = _lib.lib().gtcrn_mix_rooms_pcm16 if x.dtype == np.int16 else _lib.lib().gtcrn_mix_rooms
    _lib._check(fn(xb.data_ptr(), whole(x).shape[1], x.shape[0], ob.data_ptr(), whole(out).shape[1], out.shape[0], n, st.data_ptr(),
                   se.data_ptr(), len(seats), len(room_start) - 1, None if nr is None else nr.data_ptr(), rc.data_ptr(), rec.shape[0],
                   pr.data_ptr(), vptr, vstride, None))
    torch.cuda.synchronize()
    whole(out)[:] = ob.cpu().numpy()
    rec[:] = rc.cpu().numpy()
    assert item == xb.element_size()


@pytest.mark.parametrize("pad", [5, 0])
@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_kernel_equals_checker(dev, name, c, pcm, pad):
    MC.run(c, kernel, pcm, pad)


@pytest.mark.parametrize("name,c", POISON, ids=[n for n, _ in POISON])
def test_kernel_equals_checker_on_non_finite_blocks(dev, name, c):
    MC.run(c, kernel, False, 5)
    MC.run(c, kernel, False, 0)


def test_two_identical_calls_give_identical_bits(dev):
    """(the checker apart) no order in the kernel depends on timing: big rooms, many workgroups, twice."""
    c = MC.sizes_case(160, 1, big=True)
    runs = []
    for _ in range(2):
        rec = np.zeros((c["n_rec"], 4), F)
        outs = []
        for x, _, _ in c["ticks"]:
            out = np.full((x.shape[0], 160), MC.GUARD_F, F)
            kernel(x[:, :], out[:, :], c["room_start"], c["seats"], rec, c["params"], None, None)
            outs.append(out.tobytes())
        runs.append((outs, rec.tobytes()))
    assert runs[0] == runs[1]


def bridge(rooms, ticks, **kw):
    """The checker for a Mixer whose rows are the participant ids: ticks of (x, the ids absent in it); returns per-tick (out, rec)."""
    start, seats = MC.tables([[(p, p, p) for p in r] for r in rooms])
    P = ticks[0][0].shape[0]
    rec, trace = np.zeros((P, 4), F), []
    for x, absent in ticks:
        tab = seats.copy()
        for s in tab:
            if s[0] in absent:
                s[0] = -1
        out = np.zeros_like(x)
        MK.mix(x, out, start, tab, rec, MK.params(**kw))
        trace.append((out, rec.copy()))
    return trace


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_mixer_class(dev, pcm):
    from gtcrn_micro_amd import Mixer
    rng = np.random.default_rng(21)
    rooms = [[0, 1, 2], [3, 4, 5, 6, 7], [8]]
    xs = [MC.noise(rng, 9, 160, [0.02, 0.1, 0.3]) for _ in range(4)]
    if pcm:
        xs = [MC.to_pcm(x) for x in xs]
    absent = [set(), {4}, set(), {0}]
    want = bridge(rooms, list(zip(xs, absent)), k=2)
    m = Mixer(9, 4, 16, 0, k=2)
    for t, x in enumerate(xs):
        m.set_rooms(rooms, in_rows={p: p for p in range(9) if p not in absent[t]})
        out = m.mix(torch.from_numpy(x).cuda())
        assert MK.same_bits(out.cpu().numpy(), want[t][0]) and MK.same_bits(m.records().cpu().numpy(), want[t][1]), t
        assert m.selected().tolist() == (want[t][1][:, 0] == 1).tolist()
    assert want[-1][1][:, 2].sum() > 4 and 0 < m.selected().sum() < 9
    m.reset([3, 4])
    rec = m.records().cpu().numpy()
    assert not rec[3:5].any() and MK.same_bits(rec[[0, 1, 2, 5, 6, 7, 8]], want[-1][1][[0, 1, 2, 5, 6, 7, 8]])
    m.reset()
    assert not m.records().any()
    # a fresh start gives the first tick again, into a caller's buffer with a pitch
    m.set_rooms(rooms)
    buf = torch.full((9, 165), 7, device="cuda", dtype=torch.int16 if pcm else torch.float32)
    got = m.mix(torch.from_numpy(xs[0]).cuda(), out=buf[:, :160])
    assert got.data_ptr() == buf.data_ptr() and MK.same_bits(buf[:, :160].cpu().numpy(), want[0][0]) and (buf[:, 160:] == 7).all()


def test_mixer_refuses_what_the_tables_cannot_hold(dev):
    from gtcrn_micro_amd import GtcrnError, Mixer
    m = Mixer(8, 2, 6, 0)
    for rooms, kw, reason in (([[0, 1], [1, 2]], {}, "participant 1 is named twice"),
                              ([[0, 1, 2]], dict(out_rows={0: 3, 1: 3, 2: 4}), "output row 3 is named twice"),
                              ([[0, 8]], {}, "outside 0 .. 7"), ([[0], [1], [2]], {}, "the tables hold"),
                              ([[0, 1, 2, 3], [4, 5, 6]], {}, "the tables hold"), ([[0, 1]], dict(in_rows=[0, -3]), "a row is -1")):
        with pytest.raises(GtcrnError, match=reason):
            m.set_rooms(rooms, **kw)
    m.set_rooms([[0, 1, 2]], in_rows={0: 0, 1: 5})
    with pytest.raises(GtcrnError, match="input row 5"):
        m.mix(torch.zeros((4, 160), device="cuda"))
    with pytest.raises(GtcrnError, match="voice"):
        m.mix(torch.zeros((6, 160), device="cuda"), voice=torch.zeros(4, device="cuda"))
    with pytest.raises(GtcrnError, match="k must lie in 1 .. 8"):
        m.set_params(k=9)
    with pytest.raises(GtcrnError, match="overlap"):
        x = torch.zeros((12, 160), device="cuda")
        m.mix(x[:6], out=x[4:10])


def test_a_captured_call_follows_tables_parameters_and_room_count(dev):
    from gtcrn_micro_amd import Mixer
    rng = np.random.default_rng(22)
    P, n = 12, 160
    xs = [MC.noise(rng, P, n, [0.02, 0.1, 0.3]) for _ in range(5)]
    plans = [([[0, 1, 2], [3, 4, 5, 6], [7, 8, 9, 10, 11]], dict(k=3)),
             ([[0, 1, 2], [3, 4, 5, 6], [7, 8, 9, 10, 11]], dict(k=1, incumbent_db=0.0)),
             ([[7, 8, 9, 10, 11], [0, 1, 2, 3, 4, 5, 6]], dict(k=2, release=1.0)),
             ([[0, 1, 2, 3, 4, 5, 6]], dict(k=2, floor_dbov=-20.0)),
             ([[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11]], dict(k=3))]
    rec, want = np.zeros((P, 4), F), []
    for x, (rooms, kw) in zip(xs, plans):
        start, seats = MC.tables([[(p, p, p) for p in r] for r in rooms])
        out = np.zeros_like(x)
        f = dict(k=3, floor_dbov=-50.0, alpha=0.125, incumbent_db=3.0)
        f.update({("alpha" if k == "release" else k): v for k, v in kw.items()})
        MK.mix(x, out, start, seats, rec, MK.params(**f))
        want.append((out, rec.copy()))
    m = Mixer(P, 6, P, 0)
    m.set_rooms([])
    xb, ob = torch.zeros((P, n), device="cuda"), torch.zeros((P, n), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.mix(xb, out=ob)                                             # warm-up with no room: nothing is written
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.mix(xb, out=ob)
    assert not m.records().any()
    for t, (x, (rooms, kw)) in enumerate(zip(xs, plans)):
        m.set_params(**dict(dict(k=3, floor_dbov=-50.0, release=0.125, incumbent_db=3.0), **kw))
        m.set_rooms(rooms)
        xb.copy_(torch.from_numpy(x))
        ob.zero_()
        graph.replay()
        assert MK.same_bits(ob.cpu().numpy(), want[t][0]) and MK.same_bits(m.records().cpu().numpy(), want[t][1]), t
    assert len({w[1][:, 0].tobytes() for w in want}) > 2


def vad_words(eng, win, x):
    """Level-control words that only measure, with the floor at the median energy of the hops a plain state emits for x and the
    ratio test out of the way: about half of the blocks count as voiced."""
    from gtcrn_micro_amd import alc_params
    w = eng.wave_stream_step(eng.new_wave_state(x.shape[0], win), x[:, :x.shape[1] // 256 * 256].contiguous()).cpu().numpy()
    p = alc_params(mode=0, ratio_db=-60, hang_ms=0)
    e = (w.reshape(w.shape[0], -1, 256).astype(np.float64) ** 2).sum(-1)[:, 2:]
    p[0] = F(np.median(e))
    assert p[0] > 0
    return p


def speechlike(P, samples, seed):
    """Noise whose amplitude steps between 0.3, 0.01 and 1e-4 every 640 samples, the streams offset against each other."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(P, samples, device="cuda", generator=gen)
    amp = torch.tensor([[(0.3, 0.01, 1e-4)[((k + 2 * s) // 4) % 3] for k in range(samples // 160)] for s in range(P)], device="cuda")
    return x * amp.repeat_interleave(160, 1)


ROOMS = [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9, 10, 11]]
FOUR = lambda st: (st.model, st.wave, st.pkt, st.phase, st.alc)


def bridge_ticks(eng, win, warm=8, T=6):
    """Two packet-slot states of 12 slots at 16 kHz / 160 with alc="vad", warmed by `warm` packets; the six ticks' inputs and
    the slot each tick loses."""
    P, n = 12, 160
    x = speechlike(P, n * (warm + T), 31)
    words = vad_words(eng, win, x)
    states = [eng.new_packet_slot_state(P, win, n, 16000, alc="vad") for _ in range(2)]
    every = i32(range(P))
    for st in states:
        st.alc_params.copy_(torch.from_numpy(words))
        for t in range(warm):
            eng.packet_stream_step_slots(st, every, x[:, n * t:n * (t + 1)].contiguous())
    lost = [(5 * t + 1) % P for t in range(T)]
    return states, [x[:, n * (warm + t):n * (warm + t + 1)].contiguous() for t in range(T)], lost


def expected_mix(rows, act, voice, rec):
    """The checker on the GPU's own enhanced rows (row i of `rows` is slot act[i]) and voice words; rec is carried."""
    where = {s: i for i, s in enumerate(act)}
    start, seats = MC.tables([[(where.get(p, -1), p, p) for p in r] for r in ROOMS])
    out = np.zeros((12, rows.shape[1]), F)
    MK.mix(rows, out, start, seats, rec, MK.params(), voice=voice)
    return out


def test_bridge_end_to_end_behind_a_packet_slot_state(eng, win):
    from gtcrn_micro_amd import Mixer
    (st, plain), xs, lost = bridge_ticks(eng, win)
    m = Mixer(12, 3, 12, 0)
    rec, voices, gs = np.zeros((12, 4), F), [], []
    for t, x in enumerate(xs):
        act = [s for s in range(12) if s != lost[t]]
        y = eng.packet_stream_step_slots(st, i32(act), x[act].contiguous())
        m.set_rooms(ROOMS, in_rows={s: i for i, s in enumerate(act)})
        out = m.mix(y, out=torch.zeros((12, 160), device="cuda"), voice=st.alc[:, 3])
        yp = eng.packet_stream_step_slots(plain, i32(act), x[act].contiguous())
        assert torch.equal(y.view(torch.int32), yp.view(torch.int32)), t
        voice = st.alc[:, 3].cpu().numpy()
        want = expected_mix(y.cpu().numpy(), act, voice, rec)
        assert MK.same_bits(out.cpu().numpy(), want) and MK.same_bits(m.records().cpu().numpy(), rec), t
        voices.append(voice != 0)
        gs.append(rec[:, 0].tobytes())
    for a, b in zip(FOUR(st), FOUR(plain)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the mixer moved a bit of the state"
    v = np.stack(voices)
    assert v.any() and not v.all() and rec[:, 2].sum() > 0 and len(set(gs)) > 1 and (rec[:, 3] == 6).all()


def test_step_and_mix_in_one_captured_graph(eng, win):
    from gtcrn_micro_amd import Mixer
    (sg, se), xs, lost = bridge_ticks(eng, win)
    me, mg = Mixer(12, 3, 12, 0), Mixer(12, 3, 12, 0)
    eager = []
    for t, x in enumerate(xs):
        act = [s for s in range(12) if s != lost[t]]
        y = eng.packet_stream_step_slots(se, i32(act), x[act].contiguous())
        me.set_rooms(ROOMS, in_rows={s: i for i, s in enumerate(act)})
        eager.append((me.mix(y, out=torch.zeros((12, 160), device="cuda"), voice=se.alc[:, 3]).clone(), me.records()))
    slots, count = i32(range(12)), i32([0])
    xin, y, out = (torch.zeros((12, 160), device="cuda") for _ in range(3))
    mg.set_rooms([])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.packet_stream_step_slots(sg, slots, xin, count=count, out=y)      # warm-up with count 0 and no room
        mg.mix(y, out=out, voice=sg.alc[:, 3])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.packet_stream_step_slots(sg, slots, xin, count=count, out=y)
        mg.mix(y, out=out, voice=sg.alc[:, 3])
    for t, x in enumerate(xs):
        act = [s for s in range(12) if s != lost[t]]
        slots.copy_(i32(act + [lost[t]]))
        count.fill_(11)
        xin[:11].copy_(x[act])
        mg.set_rooms(ROOMS, in_rows={s: i for i, s in enumerate(act)})
        out.zero_()
        graph.replay()
        assert torch.equal(out.view(torch.int32), eager[t][0].view(torch.int32)), t
        assert torch.equal(mg.records().view(torch.int32), eager[t][1].view(torch.int32)), t
    for a, b in zip(FOUR(sg), FOUR(se)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert eager[-1][1][:, 2].sum() > 0
