"""Packet stream slots (gtcrn_packet_stream_*_slots): a call steps the resident packet streams it names, each at its own
phase.  The truth is always unchanged code -- the contiguous gtcrn_packet_stream_step on a ONE-stream group created fresh
(phase 0) and fed the same packets, or Engine.forward_wave by the header contract -- never the new calls (contract:
include/gtcrn_micro_hip.h, "packet stream slots").  Every comparison is exact."""
import ctypes
from math import gcd

import numpy as np
import pytest

from conftest import load_params
import packet_plan_emulator as PE

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S = 23            # resident slots = max_active: the narrow form spans 6 workgroups of 4, the wide form 4 of 7, ragged tails
TICKS = 40


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


def i32(ids):
    return torch.tensor(list(ids), dtype=torch.int32, device="cuda")


def padded(ids, n=S):
    """The call's slot table: `ids`, then the other slots (never read, but in range and distinct all the same)."""
    return i32(list(ids) + [s for s in range(n) if s not in ids])


def make_schedule(ticks, seed=2311):
    """Per tick the slots that have a packet, in the order the server gathered them: slot s joins at tick s % 7, then
    skips about a quarter of the ticks; every few ticks the order is left sorted, one tick is empty, one is everybody."""
    rng = np.random.default_rng(seed)
    sched = []
    for t in range(ticks):
        ids = [s for s in range(S) if t >= s % 7 and rng.random() > 0.25]
        if t == 5:
            ids = []
        if t == 8:
            ids = list(range(S))
        if t % 4:
            ids = [ids[i] for i in rng.permutation(len(ids))]
        sched.append(ids)
    return sched


SCHEDULE = make_schedule(TICKS)
SHORT = SCHEDULE[:14]


def clip(n, ticks, seed, pcm=False):
    """x (S, n ticks) seeded * 0.1 (int16: the same, rounded)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(S, n * ticks, device="cuda", generator=gen) * 0.1
    if pcm:
        from gtcrn_micro_amd import f32_to_pcm16
        x = f32_to_pcm16(x)
    return x


def test_schedule_is_what_it_claims():
    assert any(t != sorted(t) for t in SCHEDULE) and [] in SCHEDULE and list(range(S)) in SCHEDULE
    assert all(len(set(t)) == len(t) and all(0 <= s < S for s in t) for t in SCHEDULE)
    for s in range(S):
        named = sum(s in t for t in SCHEDULE)
        assert 15 <= named <= TICKS - 3, s                       # every slot steps often and skips ticks
        assert sum(s in t for t in SHORT) >= 4, s
    for n16, pair in ((160, {0, 1}), (320, {1, 2})):
        for sched in (SCHEDULE, SHORT):
            hs, phase = PE.run(S, sched, n16)
            assert any(pair <= set(h) for h in hs), (n16, "no call mixes rows of %s hops" % sorted(pair))
            assert len(set(phase)) > 2                           # the slots' phases differ
    hs, _ = PE.run(S, SCHEDULE, 256)
    assert all(set(h) <= {1} for h in hs)


def truth_for(eng, win, fs, n, packets, gains=None):
    """The contiguous packet form on a one-stream group created fresh, fed `packets` (k, n): (outputs (k n,), state).
    gains: None or a list of k dry gains (the gain in force at each call)."""
    st = eng.new_packet_state(1, win, n, fs)
    assert st.phase == 0
    g = None
    if gains is not None:
        g = torch.zeros(1, device="cuda")
        st.set_dry_gain(g)
    outs = []
    for k in range(packets.shape[0]):
        if g is not None:
            g.fill_(gains[k])
        outs.append(eng.packet_stream_step(st, packets[k:k + 1]).clone())
    return (torch.cat(outs, 1)[0] if outs else packets.new_zeros(0)), st


def run_slots(eng, win, fs, n, sched, x, st=None, gain_at=None, seen=None):
    """Steps the schedule on an S-slot state; slot s consumes x[s] packet by packet.  gain_at: {tick: (slot, gain)} written
    into st.dry_gain before that tick.  Returns (per-slot emitted output, state, per-slot packets consumed)."""
    st = st or eng.new_packet_slot_state(S, win, n, fs)
    seen = seen or [0] * S
    blocks = [[] for _ in range(S)]
    xin = torch.zeros((S, n), device="cuda", dtype=x.dtype)
    out = torch.empty((S, n), device="cuda", dtype=x.dtype)
    fill = 77 if x.dtype == torch.int16 else -7.0
    for t, ids in enumerate(sched):
        if gain_at and t in gain_at:
            st.dry_gain[gain_at[t][0]] = gain_at[t][1]
        xin.zero_()
        for i, s in enumerate(ids):
            xin[i] = x[s, n * seen[s]:n * (seen[s] + 1)]
        out.fill_(fill)
        eng.packet_stream_step_slots(st, padded(ids), xin, count=i32([len(ids)]), out=out)
        assert torch.equal(out[len(ids):], torch.full_like(out[len(ids):], fill)), "rows at or beyond count were written"
        for i, s in enumerate(ids):
            blocks[s].append(out[i].clone())
            seen[s] += 1
    return [torch.cat(b) if b else x.new_zeros(0) for b in blocks], st, seen


def assert_slots_equal_truth(eng, win, fs, n, x, got, st, seen, gains_of=None, first=None):
    """Per slot: outputs and all four states equal the one-stream truth of the packets it consumed (from packet first[s])."""
    for s in range(S):
        a = first[s] if first else 0
        pk = x[s, n * a:n * seen[s]].reshape(seen[s] - a, n)
        want, ts = truth_for(eng, win, fs, n, pk, gains_of(s) if gains_of else None)
        assert torch.equal(got[s], want), (fs, n, s)
        assert torch.equal(st.model[s:s + 1], ts.model) and torch.equal(st.wave[s:s + 1], ts.wave), (fs, n, s)
        assert torch.equal(st.pkt[s:s + 1], ts.pkt), (fs, n, s)
        assert int(st.phase[s]) == ts.phase, (fs, n, s)
    assert any(g.any() for g in got)


@pytest.fixture(scope="module")
def clips16():
    return {n: clip(n, TICKS, 100 + n) for n in (160, 320)}


@pytest.mark.parametrize("n", [160, 320])
@pytest.mark.parametrize("form", [0, 2, 3])
def test_ragged_schedule_equals_per_slot_truth_16k(eng, win, clips16, form, n):
    """40 ticks, slots joining at different ticks, skipping ticks, named in unsorted order: calls mix rows of 0 and 1 hops
    (n = 160) or 1 and 2 hops (n = 320; test_schedule_is_what_it_claims).  Outputs and all four states per slot equal the
    one-stream contiguous truth, and the outputs equal zeros(L16) ++ forward_wave(x)."""
    x = clips16[n]
    eng.stream_form(form)
    try:
        got, st, seen = run_slots(eng, win, 16000, n, SCHEDULE, x)
    finally:
        eng.stream_form(0)
    assert isinstance(st.phase, torch.Tensor) and st.phase.dtype == torch.int32 and st.latency16 == 512 - gcd(n, 256)
    assert_slots_equal_truth(eng, win, 16000, n, x, got, st, seen)
    lead = 512 - gcd(n, 256)
    for s in range(S):
        L = n * seen[s]
        Y = eng.forward_wave(x[s, :L], win)
        assert torch.equal(got[s], torch.cat([torch.zeros(lead, device="cuda"), Y[:L - lead]])), (n, s)


@pytest.mark.parametrize("fs,n", [(48000, 480), (8000, 80), (44100, 441)])
def test_ragged_schedule_at_other_rates(eng, win, fs, n):
    """The shortened schedule through the resampling stages (44.1 kHz: phase tables read from global memory)."""
    x = clip(n, len(SHORT), fs // 100 + n)
    got, st, seen = run_slots(eng, win, fs, n, SHORT, x)
    assert st.fs == fs and st.packet == n and st.n16 == n * 16000 // fs
    assert_slots_equal_truth(eng, win, fs, n, x, got, st, seen)


@pytest.mark.parametrize("fs,n", [(16000, 320), (48000, 480)])
def test_pcm16_form(eng, win, fs, n):
    x = clip(n, len(SHORT), 7 + n, pcm=True)
    got, st, seen = run_slots(eng, win, fs, n, SHORT, x)
    assert got[0].dtype == torch.int16
    assert_slots_equal_truth(eng, win, fs, n, x, got, st, seen)


@pytest.mark.parametrize("n", [160, 320])
def test_per_slot_gains_against_the_limited_truth(eng, win, n):
    """Gains by SLOT: 0 (no limit), 1 (bypass), others, and slot 2's changed at tick 7.  At n = 320 a row's second hop takes
    its dry samples from the ring."""
    x = clip(n, len(SHORT), 900 + n)
    base = [0.0 if s % 4 == 0 else (1.0 if s % 4 == 1 else 0.05 * s) for s in range(S)]
    st = eng.new_packet_slot_state(S, win, n)
    st.set_dry_gain(torch.tensor(base, device="cuda"))
    got, st, seen = run_slots(eng, win, 16000, n, SHORT, x, st=st, gain_at={7: (2, 0.75)})
    before7 = sum(2 in t for t in SHORT[:7])
    assert 0 < before7 < seen[2] and base[2] not in (0.0, 1.0, 0.75)

    def gains_of(s):
        if s != 2:
            return [base[s]] * seen[s]
        return [base[2]] * before7 + [0.75] * (seen[2] - before7)

    assert_slots_equal_truth(eng, win, 16000, n, x, got, st, seen, gains_of=gains_of)
    plain, _, _ = run_slots(eng, win, 16000, n, SHORT, x)
    assert torch.equal(plain[0], got[0]) and not torch.equal(plain[3], got[3])      # gain 0 IS no limit; 0.15 is not


def four(st):
    return [t.clone() for t in (st.model, st.wave, st.pkt, st.phase)]


@pytest.mark.parametrize("form", [2, 3])
def test_idle_slots_and_unused_rows_are_untouched(eng, win, form):
    n = 160
    x = clip(n, 8, 31)
    eng.stream_form(form)
    try:
        st = eng.new_packet_slot_state(S, win, n)
        for k in range(3):                                          # every slot holds history, phase 224
            eng.packet_stream_step_slots(st, i32(range(S)), x[:, n * k:n * (k + 1)].contiguous())
        assert set(st.phase.tolist()) == {224}
        ids = [19, 2, 11, 7, 8]
        idle = [s for s in range(S) if s not in ids]
        b0 = four(st)
        out = torch.full((S, n), -7.0, device="cuda")
        eng.packet_stream_step_slots(st, padded(ids), x[:, 3 * n:4 * n].contiguous(), count=i32([len(ids)]), out=out)
        for a, b in zip(four(st), b0):
            assert torch.equal(a[idle], b[idle])
            assert not torch.equal(a[ids], b[ids])
        assert torch.equal(out[len(ids):], torch.full_like(out[len(ids):], -7.0)) and (out[:len(ids)] != -7.0).all()
        b1 = four(st)
        out.fill_(-7.0)
        eng.packet_stream_step_slots(st, padded(ids), x[:, 4 * n:5 * n].contiguous(), count=i32([0]), out=out)
        assert all(torch.equal(a, b) for a, b in zip(four(st), b1))
        assert torch.equal(out, torch.full_like(out, -7.0))
        eng.packet_stream_reset_slots(st, padded(ids), count=i32([0]))
        assert all(torch.equal(a, b) for a, b in zip(four(st), b1))
    finally:
        eng.stream_form(0)


def test_device_count_is_clamped_to_max_active(eng, win):
    """The table, x and out are views of M + 5 valid rows; max_active = M, device count = M + 5: only M rows step.  A
    missing clamp shows as a wrong answer (the five extra rows are real rows of real buffers), never as a stray access."""
    n, M = 320, 9
    ids = [14, 3, 20, 6, 9, 1, 17, 12, 5, 22, 0, 8, 19, 11]
    x = clip(n, 3, 57)
    st = eng.new_packet_slot_state(S, win, n, max_active=M)
    ref = eng.new_packet_slot_state(S, win, n)
    for a in (st, ref):
        for lo in (0, M, 2 * M):                                    # (max_active rows a call)
            rows = list(range(S))[lo:lo + M]
            eng.packet_stream_step_slots(a, i32(rows), x[rows, :n].contiguous())
    b0 = four(st)
    xin = x[ids, n:2 * n].contiguous()
    out = torch.full((M + 5, n), -7.0, device="cuda")
    table = i32(ids)
    eng.packet_stream_step_slots(st, table[:M], xin[:M], count=i32([M + 5]), out=out[:M])
    untouched = [s for s in range(S) if s not in ids[:M]]
    for a, b in zip(four(st), b0):
        assert torch.equal(a[untouched], b[untouched])
    assert torch.equal(out[M:], torch.full_like(out[M:], -7.0))
    want = eng.packet_stream_step_slots(ref, i32(ids[:M]), xin[:M])
    assert torch.equal(out[:M], want) and all(torch.equal(a, b) for a, b in zip(four(st), four(ref)))
    from gtcrn_micro_amd import GtcrnError
    with pytest.raises(GtcrnError):
        eng.packet_stream_step_slots(st, table[:M + 1], xin[:M + 1])          # more rows than max_active


def test_leave_and_rejoin_by_the_reset_kernel(eng, win):
    """Ten ticks; slots 4 and 11 then leave, are reset by the kernel while the others run on, and start new clips: their
    second lives equal a fresh one-stream truth, everybody else their uninterrupted one."""
    n = 160
    x = clip(n, TICKS, 404)
    got1, st, seen = run_slots(eng, win, 16000, n, SCHEDULE[:10], x)
    left = [11, 4]
    away = [[s for s in t if s not in left] for t in SCHEDULE[10:14]]
    got2, st, seen = run_slots(eng, win, 16000, n, away, x, st=st, seen=seen)
    assert all(int(st.phase[s]) for s in left)                              # they left mid-hop
    eng.packet_stream_reset_slots(st, i32(left))
    assert not st.phase[left].any() and not st.pkt[left].any() and not st.model[left].any() and not st.wave[left].any()
    first = [seen[s] if s in left else 0 for s in range(S)]
    got3, st, seen = run_slots(eng, win, 16000, n, SCHEDULE[14:28], x, st=st, seen=list(seen))
    got = [g3 if s in left else torch.cat([g1, g2, g3]) for s, (g1, g2, g3) in enumerate(zip(got1, got2, got3))]
    assert_slots_equal_truth(eng, win, 16000, n, x, got, st, seen, first=first)


def test_one_captured_call_serves_every_phase_and_active_set(eng, win):
    """ONE capture of ONE call (n = 160: a period is 8 ticks), replayed for 20 ticks with the table, the count, the packets
    and a gain rewritten between replays, equals the eager run: the launch sequence does not depend on any phase."""
    n, M = 160, 13
    x = clip(n, 20, 606)
    rng = np.random.default_rng(5)
    ticks = [(rng.permutation(S)[:M], c) for c in [13, 0, 5, 13, 1, 7, 4, 0, 12, 8, 13, 3, 9, 13, 2, 11, 6, 13, 10, 5]]
    assert len(ticks) > 2 * (256 // gcd(n, 256))
    seen = [0] * S
    inputs = []
    for perm, c in ticks:
        xin = torch.zeros((M, n), device="cuda")
        for i in range(c):
            s = int(perm[i])
            xin[i] = x[s, n * seen[s]:n * (seen[s] + 1)]
            seen[s] += 1
        inputs.append(xin)
    gains = lambda k: 0.25 if k < 9 else 0.6          # noqa: E731   (slot 3's gain changes at tick 9)

    def fresh():
        st = eng.new_packet_slot_state(S, win, n, max_active=M)
        st.set_dry_gain(torch.zeros(S, device="cuda"))
        return st

    se = fresh()
    eager = []
    for k, ((p, c), xin) in enumerate(zip(ticks, inputs)):
        se.dry_gain[3] = gains(k)
        eager.append(eng.packet_stream_step_slots(se, i32(p), xin, count=i32([c])).clone()[:c])
    assert len(set(se.phase.tolist())) > 2
    sg = fresh()
    slots, count = i32(ticks[0][0]), i32([0])
    xin, out = torch.zeros((M, n), device="cuda"), torch.zeros((M, n), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.packet_stream_step_slots(sg, slots, xin, count=count, out=out)    # warm-up with count 0: nothing steps
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.packet_stream_step_slots(sg, slots, xin, count=count, out=out)
    for k, ((p, c), xk) in enumerate(zip(ticks, inputs)):
        slots.copy_(i32(p))
        count.fill_(c)
        xin.copy_(xk)
        sg.dry_gain[3] = gains(k)
        graph.replay()
        assert torch.equal(out[:c], eager[k]), k
    assert all(torch.equal(a, b) for a, b in zip(four(sg), four(se)))


def _launches(eng, fn):
    eng.timing_enable(True)
    fn()
    torch.cuda.synchronize()
    t = {k: v[1] for k, v in eng.timing_read().items()}
    eng.timing_enable(False)
    return t


@pytest.mark.parametrize("fs,n", [(16000, 160), (16000, 320), (48000, 480)])
def test_every_call_makes_the_same_launch_sequence(eng, win, fs, n):
    """From the library's launch records: plan, inbound, hmax single-launch indexed wave steps, outbound -- whatever the
    phases and the active set, and never a multi-frame kernel (16 kHz / 320 steps two hops as two one-frame launches)."""
    n16 = n * 16000 // fs
    hmax = PE.hmax_of(n16)
    assert hmax == (2 if n == 320 else 1)
    for k in ("k_packet_plan", "k_packet_in_slots", "k_packet_out_slots"):
        assert k in eng.kernel_names()
    st = eng.new_packet_slot_state(S, win, n, fs)
    x = clip(n, 1, 9)
    y = torch.empty_like(x)
    seen = []
    for t, ids in enumerate(SCHEDULE[:10]):
        got = _launches(eng, lambda: eng.packet_stream_step_slots(st, padded(ids), x, count=i32([len(ids)]), out=y))
        seen.append(got)
        assert not any(k in got for k in ("k_encoder", "k_gtcn1", "k_gtcn2", "k_gtcn_ms", "k_decoder", "k_packet_in",
                                          "k_packet_out")), got
    assert all(g == seen[0] for g in seen), seen
    model = [k for k in seen[0] if k in ("k_stream_ms", "k_stream_wide")]
    assert len(model) == 1
    assert seen[0] == {"k_packet_plan": 1, "k_packet_in_slots": 1, "k_packet_out_slots": 1, "k_wave_analysis": hmax,
                       model[0]: hmax, "k_wave_synthesis": hmax}
    assert len(set(st.phase.tolist())) > 1


def test_error_paths_leave_the_states_alone(eng, win):
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import lib
    n, M = 160, 4
    st = eng.new_packet_slot_state(S, win, n, max_active=M)
    x = clip(n, 2, 3)
    eng.packet_stream_step_slots(st, i32([3, 9, 1, 20]), x[[3, 9, 1, 20], :n].contiguous())
    b0 = four(st)
    out = torch.full((M, n), -7.0, device="cuda")
    good, hop = i32([3, 9, 1, 20]), x[:M, n:].contiguous()
    L, sp = lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    m, w, p, ph, sl, xi, o, wi = (st.model.data_ptr(), st.wave.data_ptr(), st.pkt.data_ptr(), st.phase.data_ptr(),
                                  good.data_ptr(), hop.data_ptr(), out.data_ptr(), st.window.data_ptr())
    step, reset = L.gtcrn_packet_stream_step_slots, L.gtcrn_packet_stream_reset_slots
    calls = [
        lambda: step(None, m, w, p, ph, sl, None, M, xi, n, o, n, wi, sp),
        lambda: step(st._h, None, w, p, ph, sl, None, M, xi, n, o, n, wi, sp),
        lambda: step(st._h, m, None, p, ph, sl, None, M, xi, n, o, n, wi, sp),
        lambda: step(st._h, m, w, None, ph, sl, None, M, xi, n, o, n, wi, sp),
        lambda: step(st._h, m, w, p, None, sl, None, M, xi, n, o, n, wi, sp),
        lambda: step(st._h, m, w, p, ph, None, None, M, xi, n, o, n, wi, sp),
        lambda: step(st._h, m, w, p, ph, sl, None, M, None, n, o, n, wi, sp),
        lambda: step(st._h, m, w, p, ph, sl, None, M, xi, n, None, n, wi, sp),
        lambda: step(st._h, m, w, p, ph, sl, None, M, xi, n, o, n, None, sp),
        lambda: step(st._h, m, w, p, ph, sl, None, 0, xi, n, o, n, wi, sp),
        lambda: step(st._h, m, w, p, ph, sl, None, M + 1, xi, n, o, n, wi, sp),       # above the handle's max_streams
        lambda: step(st._h, m, w, p, ph, sl, None, M, xi, n - 1, o, n, wi, sp),       # short strides
        lambda: step(st._h, m, w, p, ph, sl, None, M, xi, n, o, n - 1, wi, sp),
        lambda: step(st._h, m, w, p + 4, ph, sl, None, M, xi, n, o, n, wi, sp),       # states off the 16-byte grid
        lambda: step(st._h, m + 8, w, p, ph, sl, None, M, xi, n, o, n, wi, sp),
        lambda: L.gtcrn_packet_stream_step_slots_pcm16(st._h, m, w, p, ph, sl, None, M + 1, xi, n, o, n, wi, sp),
        lambda: reset(None, m, w, p, ph, sl, None, M, sp),
        lambda: reset(st._h, m, w, None, ph, sl, None, M, sp),
        lambda: reset(st._h, m, w, p, None, sl, None, M, sp),
        lambda: reset(st._h, m, w, p, ph, None, None, M, sp),
        lambda: reset(st._h, m, w, p, ph, sl, None, M + 1, sp),
        lambda: reset(st._h, m, w + 4, p, ph, sl, None, M, sp),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i                                          # GTCRN_ERR_ARG
        assert L.gtcrn_last_error(), i
    eng.stream_form(1)
    try:
        assert step(st._h, m, w, p, ph, sl, None, M, xi, n, o, n, wi, sp) == -4      # GTCRN_ERR_STATE
        with pytest.raises(GtcrnError):
            eng.packet_stream_step_slots(st, good, hop, out=out)
    finally:
        eng.stream_form(0)
    plain = eng.new_packet_state(S, win, n)
    bad = [
        lambda: eng.wave_stream_step_slots(plain, good, x[:M, :256].contiguous()),       # a plain packet state with slots=
        lambda: eng.packet_stream_step_slots(plain, good, hop, out=out),
        lambda: eng.wave_stream_step_slots(st, good, x[:M, :256].contiguous()),          # the slot state is not a wave state
        lambda: eng.packet_stream_step(st, x[:, :n].contiguous()),                       # ... nor a contiguous group
        lambda: eng.packet_stream_step_slots(st, good.long(), hop, out=out),
        lambda: eng.packet_stream_step_slots(st, good, x[:M, :256].contiguous(), out=out),
        lambda: eng.packet_stream_step_slots(st, good, x[:M + 1, :n].contiguous(), out=out),
        lambda: eng.packet_stream_step_slots(st, good, hop, count=torch.tensor([4]).cuda(), out=out),
        lambda: eng.packet_stream_reset_slots(plain, good),
        lambda: eng.new_packet_slot_state(S, win, n, max_active=S + 1),
    ]
    for i, c in enumerate(bad):
        with pytest.raises(GtcrnError):
            c()
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, -7.0))
    assert all(torch.equal(a, b) for a, b in zip(four(st), b0))
    assert not plain.wave.any() and not plain.pkt.any() and plain.phase == 0


def test_streaming_wrapper_dispatches_on_the_state_type(win):
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import PacketSlotState, PacketStreamState
    from gtcrn_micro_amd.streaming.gtcrn_micro_stream import StreamGTCRNMicro
    stream = StreamGTCRNMicro().cuda().eval()
    n = 441
    x = clip(n, 6, 12)
    st = stream.init_wave_state(S, win, fs=44100, packet=n, resident=True)
    assert isinstance(st, PacketSlotState) and isinstance(st, PacketStreamState) and st.n16 == 160 and st.latency16 == 544
    rows = [5, 18, 2]
    e = stream.engine(x.device)
    truth = e.new_packet_slot_state(S, win, n, 44100)
    for k in range(4):
        pk = x[rows, n * k:n * (k + 1)].contiguous()
        assert torch.equal(stream.step_wave(pk, st, slots=i32(rows)), e.packet_stream_step_slots(truth, i32(rows), pk)), k
    assert stream.init_wave_state(S, win, state=st, slots=i32([18])) is st
    assert int(st.phase[18]) == 0 and int(st.phase[5]) == 128 and not st.pkt[18].any()
    with pytest.raises(GtcrnError):
        stream.step_wave(x[:3, :160].contiguous(), stream.init_wave_state(S, win, packet=160), slots=i32(rows))
