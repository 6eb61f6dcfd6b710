"""Packet loss concealment on the device (include/gtcrn_micro_hip.h, "packet loss concealment"): the kernel
against the contract in numpy (tests/plc_checker.py), bit for bit, over the cases the host twins run (tests/plc_cases.py), in
float, int16 and both G.711 laws; then the Concealer class, one captured call whose flags, slots, count and parameters are
rewritten between replays, and the tick end to end in front of a packet-slot state and with the Mixer behind it."""
import numpy as np
import pytest
import torch

from conftest import load_params
import g711_checker as G
import mixer_checker as MK
import mixer_cases as MC
import plc_checker as PK
import plc_cases as PC

pytestmark = pytest.mark.gpu
F = np.float32
CASES = PC.all_cases()
TORCH = {"f32": torch.float32, "pcm16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}


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
    return torch.tensor(np.asarray(v, np.int32).reshape(-1), dtype=torch.int32, device="cuda")


def whole(v):
    """The buffer a row view was cut from."""
    return v if v.base is None else v.base


def kernel(x, lost, hist, rec, prm, slots, count, law):
    """The raw entry on device copies of the very buffers (row and history pitch included); x, hist and rec are copied back."""
    from gtcrn_micro_amd import _lib
    L = _lib.lib()
    xb, hb, rb = torch.from_numpy(whole(x).copy()).cuda(), torch.from_numpy(hist.copy()).cuda(), torch.from_numpy(rec.copy()).cuda()
    lo, pr = i32(lost), i32(prm)
    sl = None if slots is None else i32(slots)
    ct = None if count is None else i32([count])
    fn = {np.dtype(np.float32): L.gtcrn_plc_rows, np.dtype(np.int16): L.gtcrn_plc_rows_pcm16, np.dtype(np.uint8): L.gtcrn_plc_rows_g711}[x.dtype]
    args = [xb.data_ptr(), whole(x).shape[1], x.shape[0], x.shape[1], None if sl is None else sl.data_ptr(), lo.data_ptr(),
            None if ct is None else ct.data_ptr(), hb.data_ptr(), hist.shape[1], rb.data_ptr(), rec.shape[0], pr.data_ptr()]
    if x.dtype == np.uint8:
        args.append(law)
    _lib._check(fn(*args, None))
    torch.cuda.synchronize()
    whole(x)[:] = xb.cpu().numpy()
    hist[:] = hb.cpu().numpy()
    rec[:] = rb.cpu().numpy()


@pytest.mark.parametrize("pad", [5, 0])
@pytest.mark.parametrize("kind", PC.KINDS)
@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_kernel_equals_checker(dev, name, c, kind, pad):
    PC.run(c, kernel, kind, pad)


def test_kernel_equals_checker_on_non_finite_rows(dev):
    for _, c in PC.poison_cases():
        PC.run(c, kernel, "f32", 5)
        PC.run(c, kernel, "f32", 0)


def stream_rows(kind, S, n, T, fs=16000, seed=40):
    """(T, S, n) rows of the kind under test: the named signals, one per stream."""
    sig = PC.signals(fs, T * n, seed)
    x = np.stack([sig[(k + 3) % len(sig)][1] for k in range(S)])
    return np.stack([PC.as_kind(x[:, t * n:(t + 1) * n], kind) for t in range(T)])


def test_two_identical_calls_give_identical_bits(dev):
    """(the checker apart) no order in the kernel depends on timing: 23 streams, new erasures in every second tick, twice."""
    from gtcrn_micro_amd import Concealer
    rows = stream_rows("f32", 23, 480, 8, fs=48000)
    runs = []
    for _ in range(2):
        c = Concealer(23, 48000, 480, 0, torch.float32)
        outs = []
        for t in range(8):
            x = torch.from_numpy(rows[t]).cuda()
            c.conceal(x, [int(t % 2 == 1 and s % 3 != 0) for s in range(23)])
            outs.append(x.cpu().numpy().tobytes())
        runs.append((outs, c.hist.cpu().numpy().tobytes(), c.rec.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]
    assert c.events()[:, 0].sum() > 20


def test_rows_beyond_count_and_unnamed_slots_are_untouched(dev):
    from gtcrn_micro_amd import Concealer
    c = Concealer(9, 16000, 160, 0, torch.int16)
    rows = stream_rows("pcm16", 9, 160, 6)
    for t in range(4):
        c.conceal(torch.from_numpy(rows[t]).cuda(), [0] * 9)
    hist0, rec0 = c.hist.clone(), c.rec.clone()
    buf = torch.full((6, 165), 12345, dtype=torch.int16, device="cuda")
    buf[:, :160] = torch.from_numpy(rows[4][:6]).cuda()
    before = buf.clone()
    c.conceal(buf[:, :160], i32([1, 0, 1, 1, 0, 1]), slots=i32([7, 2, 5, 0, 1, 3]), count=i32([3]))
    assert torch.equal(buf[3:], before[3:]) and torch.equal(buf[:, 160:], before[:, 160:])
    assert torch.equal(buf[1], before[1]) and not torch.equal(buf[0], before[0]) and not torch.equal(buf[2], before[2])
    named = [7, 2, 5]
    others = [s for s in range(9) if s not in named]
    assert torch.equal(c.hist[others], hist0[others]) and torch.equal(c.rec[others], rec0[others])
    assert not torch.equal(c.hist[named], hist0[named]) and (c.erased()[[7, 5]] == 160).all() and int(c.erased()[2]) == 0
    c.conceal(buf[:, :160], i32([1] * 6), slots=i32([7, 2, 5, 0, 1, 3]), count=i32([0]))
    assert torch.equal(c.hist[others], hist0[others]) and int(c.events()[:, 1].sum()) == 2


@pytest.mark.parametrize("kind", PC.KINDS)
def test_concealer_class(dev, kind):
    from gtcrn_micro_amd import Concealer
    S, n, T, fs = 7, 160, 10, 8000 if kind in ("ulaw", "alaw") else 16000
    law = PC.LAW[kind]
    rows = stream_rows(kind, S, n, T, fs)
    loss = np.zeros((T, S), np.int32)
    loss[4, 1] = loss[4:7, 2] = loss[2, 3] = loss[8, 3] = loss[0, 4] = 1
    prm = PK.params(fs, hold_ms=5, fade_ms=20, recover_ms=2)
    Lh = PK.hist_len(prm)
    hist, rec = np.zeros((S, Lh), np.int16), np.zeros((S, 4), np.int32)
    c = Concealer(S, fs, n, 0, TORCH[kind], g711=None if law is None else G.NAMES[law])
    c.set_params(hold_ms=5, fade_ms=20, recover_ms=2)
    assert c.history_len == Lh and c.hist.shape == (S, Lh)
    for t in range(T):
        want = rows[t].copy()
        PK.conceal(want, loss[t], hist, rec, prm, law=law)
        x = torch.from_numpy(rows[t].copy()).cuda()
        assert c.conceal(x, i32(loss[t])) is x
        assert PK.same_bits(x.cpu().numpy(), want), t
        assert PK.same_bits(c.rec.cpu().numpy(), rec) and PK.same_bits(c.history().cpu().numpy(), PK.history(hist, rec, prm)), t
        assert c.erased().tolist() == rec[:, 2].tolist() and c.lag().tolist() == rec[:, 1].tolist()
        assert c.events().tolist() == [[int(e) & 0xFFFF, (int(e) >> 16) & 0xFFFF] for e in rec[:, 3]]
    assert rec[:, 3].tolist() == [0, 0x10001, 0x30001, 0x20002, 0x10001, 0, 0]
    c.reset([2, 3])
    assert not c.hist[2:4].any() and not c.rec[2:4].any()
    keep = [0, 1, 4, 5, 6]
    assert PK.same_bits(c.rec[keep].cpu().numpy(), rec[keep]) and PK.same_bits(c.hist[keep].cpu().numpy(), hist[keep])
    c.reset(i32([4, 0, 1]), count=i32([1]))
    assert not c.rec[4].any() and PK.same_bits(c.rec[[0, 1]].cpu().numpy(), rec[[0, 1]])
    c.reset()
    assert not c.hist.any() and not c.rec.any()
    x = torch.from_numpy(rows[0].copy()).cuda()                   # a fresh stream conceals with zeros
    c.conceal(x, [1] * S)
    zero = PC.as_kind(np.zeros((S, n), np.int16), kind)
    assert PK.same_bits(x.cpu().numpy(), zero) and (c.lag() == int(prm[1])).all()


def test_concealer_refusals(dev):
    from gtcrn_micro_amd import Concealer, GtcrnError
    for args, kw, reason in (((4, 16000, 160, "cpu", torch.float32), {}, "no CPU path"), ((4, 16000, 0, 0, torch.float32), {}, "n must lie"),
                             ((4, 16000, 1025, 0, torch.float32), {}, "n must lie"), ((4, 11025, 160, 0, torch.float32), {}, "fs must be one of"),
                             ((4, 8000, 160, 0, torch.uint8), {}, "G.711 codes"), ((4, 8000, 160, 0, torch.int16), dict(g711="ulaw"), "goes with"),
                             ((4, 8000, 160, 0, torch.float64), {}, "dtype must be"), ((0, 8000, 160, 0, torch.int16), {}, "streams must be"),
                             ((4, 8000, 160, 0, torch.int16), dict(fade_ms=0), "fade_ms must lie in 1 .. 200"),
                             ((4, 8000, 160, 0, torch.int16), dict(hold_ms=201), "hold_ms must lie in 0 .. 200"),
                             ((4, 8000, 160, 0, torch.uint8), dict(g711="law"), "g711 must be")):
        with pytest.raises(GtcrnError, match=reason):
            Concealer(*args, **kw)
    c = Concealer(4, 16000, 160, 0, torch.float32)
    x = torch.zeros((4, 160), device="cuda")
    for bad, kw, reason in ((x.to(torch.int16), {}, "made for torch.float32"), (torch.zeros((4, 80), device="cuda"), {}, "made for n = 160"),
                            (x.cpu(), {}, "tensor on cuda"), (torch.zeros((5, 160), device="cuda"), {}, "holds 4 streams"),
                            (x, dict(slots=[0, 1, 1, 2]), "names a stream twice"), (x, dict(slots=[0, 1, 2, 4]), "slots must lie in 0 .. 3"),
                            (x, dict(slots=i32([0, 1])), "at least 4 words"), (torch.zeros((160, 4), device="cuda").t(), {}, "contiguous")):
        with pytest.raises(GtcrnError, match=reason):
            c.conceal(bad, kw.pop("lost", [0] * bad.shape[0]), **kw)
    with pytest.raises(GtcrnError, match="at least 4 words"):
        c.conceal(x, i32([0, 0]))
    with pytest.raises(GtcrnError, match="recover_ms must lie in 0 .. 200"):
        c.set_params(recover_ms=-1)
    with pytest.raises(GtcrnError, match="unknown concealment fields"):
        c.set_params(comfort_noise=1)


def test_one_captured_call_follows_flags_slots_count_and_parameters(dev):
    from gtcrn_micro_amd import Concealer
    S, M, n, T = 9, 6, 160, 12
    rng = np.random.default_rng(50)
    rows = stream_rows("pcm16", S, n, T)
    plans = []
    for t in range(T):
        kw = dict(hold_ms=(10, 0, 20)[t % 3], fade_ms=(50, 10)[t % 2], recover_ms=(5, 0, 1)[(t // 2) % 3])
        plans.append((rng.permutation(S)[:M].astype(np.int32), (rng.random(M) < 0.35).astype(np.int32), (M, M, 4, M, 0, M)[t % 6], kw))
    Lh = PK.hist_len(PK.params(16000))
    hist, rec, want = np.zeros((S, Lh), np.int16), np.zeros((S, 4), np.int32), []
    for t, (ids, lost, count, kw) in enumerate(plans):
        x = rows[t][ids].copy()
        PK.conceal(x, lost, hist, rec, PK.params(16000, **kw), ids, count)
        want.append((x, hist.copy(), rec.copy()))
    c = Concealer(S, 16000, n, 0, torch.int16)
    xb, lo, sl, ct = torch.zeros((M, n), dtype=torch.int16, device="cuda"), i32([0] * M), i32(range(M)), i32([0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.conceal(xb, lo, slots=sl, count=ct)                      # warm-up with count 0: nothing is written
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.conceal(xb, lo, slots=sl, count=ct)
    assert not c.rec.any() and not c.hist.any()
    for t, (ids, lost, count, kw) in enumerate(plans):
        c.set_params(**kw)
        xb.copy_(torch.from_numpy(rows[t][ids]))
        lo.copy_(i32(lost)); sl.copy_(i32(ids)); ct.fill_(count)
        graph.replay()
        assert PK.same_bits(xb.cpu().numpy(), want[t][0]), t
        assert PK.same_bits(c.hist.cpu().numpy(), want[t][1]) and PK.same_bits(c.rec.cpu().numpy(), want[t][2]), t
    assert (rec[:, 3] & 0xFFFF).sum() > 4


def test_a_nan_row_moves_no_bit_of_another_stream(dev):
    from gtcrn_micro_amd import Concealer
    runs = []
    for poisoned in (False, True):
        case = PC.poison_case(poisoned)
        c = Concealer(8, 16000, 160, 0, torch.float32)
        outs = []
        for rows, lost, _, _ in case["ticks"]:
            x = torch.from_numpy(rows.copy()).cuda()
            c.conceal(x, i32(lost))
            outs.append(x.cpu().numpy())
        runs.append((np.stack(outs), c.history().cpu().numpy(), c.rec.cpu().numpy()))
    others = [0, 1, 3, 4, 5, 6, 7]
    for a, b in zip(*runs):
        a, b = (a[:, others], b[:, others]) if a.ndim == 3 else (a[others], b[others])
        assert PK.same_bits(a, b)
    assert not PK.same_bits(runs[0][0][:, 2], runs[1][0][:, 2]) and np.isnan(runs[1][0][:, 2]).any()
    assert (runs[1][1][2] == -32768).any()


# ---- the tick end to end: conceal -> step -> mix ---------------------------------------------------------------------------------
P = 12
ROOMS = [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9, 10, 11]]
STATE = lambda st: (st.model, st.wave, st.pkt, st.phase, st.alc)


def tick_inputs(kind, fs, n, T, warm=8):
    sig = PC.signals(fs, (T + warm) * n, 60)
    x = np.stack([sig[5 + (k % 2)][1] if k % 3 else np.roll(sig[5][1], 977 * k) for k in range(P)])
    x = np.stack([np.roll(v, 311 * k) for k, v in enumerate(x)])
    rows = np.stack([PC.as_kind(x[:, t * n:(t + 1) * n], kind) for t in range(T + warm)])
    lost = np.zeros((T + warm, P), np.int32)
    for t in range(T):
        lost[warm + t, (5 * t + 1) % P] = 1
    lost[warm + 2:warm + 5, 9] = 1                                 # one slot loses three in a row
    return rows, lost, warm


@pytest.mark.parametrize("kind,fs", [("f32", 16000), ("ulaw", 8000)])
def test_conceal_then_packet_slot_step(eng, win, kind, fs):
    from gtcrn_micro_amd import Concealer
    n, T = 160, 8
    law = PC.LAW[kind]
    name = None if law is None else G.NAMES[law]
    rows, lost, warm = tick_inputs(kind, fs, n, T)
    prm = PK.params(fs)
    hist, rec = np.zeros((P, PK.hist_len(prm)), np.int16), np.zeros((P, 4), np.int32)
    st, ref = (eng.new_packet_slot_state(P, win, n, fs, g711=name) for _ in range(2))
    c = Concealer(P, fs, n, 0, TORCH[kind], g711=name)
    every = i32(range(P))
    for t in range(warm + T):
        want = rows[t].copy()
        PK.conceal(want, lost[t], hist, rec, prm, law=law)
        x = torch.from_numpy(rows[t].copy()).cuda()
        c.conceal(x, i32(lost[t]), slots=every)
        y = eng.packet_stream_step_slots(st, every, x)
        yr = eng.packet_stream_step_slots(ref, every, torch.from_numpy(want).cuda())
        assert PK.same_bits(x.cpu().numpy(), want), t
        assert PK.same_bits(y.cpu().numpy(), yr.cpu().numpy()), t
    for a, b in zip((st.model, st.wave, st.pkt, st.phase), (ref.model, ref.wave, ref.pkt, ref.phase)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert PK.same_bits(c.rec.cpu().numpy(), rec) and PK.same_bits(c.hist.cpu().numpy(), hist)
    assert ((rec[:, 3] >> 16) & 0xFFFF).sum() == T + 3 - 1 and (rec[:, 3] & 0xFFFF).max() >= 1


def test_conceal_step_and_mix_in_one_captured_graph(eng, win):
    """The tick with the Mixer behind it (alc="vad"): every leg is stepped in every tick, so the leg that lost its packet stays
    in its room's mix for that block."""
    from gtcrn_micro_amd import Concealer, Mixer, alc_params
    n, T, fs = 160, 8, 16000
    rows, lost, warm = tick_inputs("f32", fs, n, T)
    words = alc_params(mode=0, ratio_db=-60, hang_ms=0)
    words[0] = F(1e-7)                                            # the voice flag: every block of these signals counts as speech
    prm = PK.params(fs)
    hist, rec = np.zeros((P, PK.hist_len(prm)), np.int16), np.zeros((P, 4), np.int32)
    sg, se = (eng.new_packet_slot_state(P, win, n, fs, alc="vad") for _ in range(2))
    for st in (sg, se):
        st.alc_params.copy_(torch.from_numpy(words))
    every = i32(range(P))
    cg, mg, me = Concealer(P, fs, n, 0, torch.float32), Mixer(P, 3, P, 0), Mixer(P, 3, P, 0)
    me.set_rooms(ROOMS)
    xin, y, out = (torch.zeros((P, n), device="cuda") for _ in range(3))
    lo, count = i32([0] * P), i32([0])
    mg.set_rooms([])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up with count 0 and no room
        cg.conceal(xin, lo, slots=every, count=count)
        eng.packet_stream_step_slots(sg, every, xin, count=count, out=y)
        mg.mix(y, out=out, voice=sg.alc[:, 3])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cg.conceal(xin, lo, slots=every, count=count)
        eng.packet_stream_step_slots(sg, every, xin, count=count, out=y)
        mg.mix(y, out=out, voice=sg.alc[:, 3])
    mg.set_rooms(ROOMS)
    count.fill_(P)
    picked = []
    for t in range(warm + T):
        want = rows[t].copy()
        PK.conceal(want, lost[t], hist, rec, prm)
        ye = eng.packet_stream_step_slots(se, every, torch.from_numpy(want).cuda())
        oe = me.mix(ye, out=torch.zeros((P, n), device="cuda"), voice=se.alc[:, 3])
        xin.copy_(torch.from_numpy(rows[t]))
        lo.copy_(i32(lost[t]))
        out.zero_()
        graph.replay()
        assert PK.same_bits(xin.cpu().numpy(), want), t
        assert torch.equal(y.view(torch.int32), ye.view(torch.int32)) and torch.equal(out.view(torch.int32), oe.view(torch.int32)), t
        assert torch.equal(mg.records().view(torch.int32), me.records().view(torch.int32)), t
        if lost[t].any():
            g = mg.records()[:, 0].cpu().numpy()
            picked.append(bool(g[np.nonzero(lost[t])[0]].any()))
            assert (mg.records()[:, 3] == t + 1).all()             # every leg, the lost one too, was in its room this block
    for a, b in zip(STATE(sg), STATE(se)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert PK.same_bits(cg.rec.cpu().numpy(), rec) and any(picked)
