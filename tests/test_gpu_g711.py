"""G.711 payloads on the packet form, the packet slots and the bulk converters (include/gtcrn_micro_hip.h, "G.711 payloads").
The truth is always unchanged code and the independent checker: the FLOAT call fed D_law[c] / 32768, its output through the
library's own f32_to_pcm16 and then tests/g711_checker.py's encoder (thresholds by np.searchsorted) -- never the new calls.
Every comparison is exact."""
import ctypes
from math import gcd

import numpy as np
import pytest

from conftest import load_params
import g711_checker as GC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ALL_P = np.arange(-32768, 32768, dtype=np.int64)
CALLS = 12
GROUP_CASES = [(law, fs, n) for law in GC.LAWS for fs, n in ((8000, 80), (8000, 160), (16000, 160))]


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


@pytest.fixture(scope="module")
def ref(dev):
    """The checker's tables, computed once: {law: (D int64[256], D / 32768 float32[256], E uint8[65536])} on the device."""
    out = {}
    for law in GC.LAWS:
        D = GC.decode_table(law)
        out[law] = (torch.from_numpy(D.astype(np.int64)).cuda(),
                    torch.from_numpy(D.astype(np.float32) / np.float32(32768.0)).cuda(),
                    torch.from_numpy(GC.encode(law, ALL_P)).cuda())
    return out


def i32(ids):
    return torch.tensor(list(ids), dtype=torch.int32, device="cuda")


def rand_codes(rows, cols, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (rows, cols), device="cuda", generator=gen, dtype=torch.int32).to(torch.uint8)


def dec(ref, law, codes):
    return ref[law][1][codes.long()]


def enc(ref, law, y):
    """E_law of the library's own PCM16 rounding of the float tensor y (numel a multiple of 8, or empty)."""
    from gtcrn_micro_amd import f32_to_pcm16
    if y.numel() == 0:
        return torch.empty(y.shape, dtype=torch.uint8, device=y.device)
    pcm = f32_to_pcm16(y.contiguous())
    return ref[law][2][pcm.long() + 32768]


def zero_code(law):
    return GC.ZERO_CODE[law]


# ---------------------------------------------------------------------------------------------- 1. bulk converters, exhaustive
@pytest.mark.parametrize("law", GC.LAWS)
def test_bulk_decode_every_code(dev, ref, law):
    from gtcrn_micro_amd import g711_to_f32
    codes = torch.arange(256, device="cuda", dtype=torch.int32).to(torch.uint8).repeat(3)       # 768 = 48 * 16
    got = g711_to_f32(codes, GC.NAMES[law])
    want = ref[law][1].repeat(3)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(g711_to_f32(codes.view(3, 256), law).view(-1), got)                       # (0 / 1 name the laws too)


@pytest.mark.parametrize("law", GC.LAWS)
def test_bulk_encode_every_int16_and_the_edges(dev, ref, law):
    from gtcrn_micro_amd import f32_to_g711, f32_to_pcm16
    exact = torch.from_numpy((ALL_P / 32768.0).astype(np.float32)).cuda()
    got = f32_to_g711(exact, GC.NAMES[law])
    assert got.dtype == torch.uint8 and torch.equal(got, ref[law][2])
    # half-way points (ties go to even), beyond full scale, both zeros, and every decode level one float ulp to each side
    lv = GC.decode_table(law).astype(np.float32) / np.float32(32768.0)
    edges = np.concatenate([
        ((ALL_P + 0.5) / 32768.0).astype(np.float32),
        np.array([1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 1e9, -1e9, np.inf, -np.inf, 0.0, -0.0, 1e-30, -1e-30], np.float32),
        np.nextafter(lv, np.float32(np.inf)), np.nextafter(lv, np.float32(-np.inf)), lv])
    edges = np.concatenate([edges, np.zeros(-len(edges) % 16, np.float32)])
    v = torch.from_numpy(edges).cuda()
    pcm = f32_to_pcm16(v)
    assert torch.equal(pcm.cpu(), torch.from_numpy(GC.pcm16(edges)).to(torch.int16))            # (the PCM16 rounding itself)
    assert torch.equal(f32_to_g711(v, law), ref[law][2][pcm.long() + 32768])
    out = torch.full((len(edges) + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    f32_to_g711(v, law, out=out[:len(edges)])
    assert (out[len(edges):] == 0xAA).all()                                                      # nothing past n is written


def test_bulk_argument_errors(dev):
    from gtcrn_micro_amd import GtcrnError, f32_to_g711, g711_to_f32
    from gtcrn_micro_amd._lib import lib
    L, sp = lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    codes = torch.zeros(64, dtype=torch.uint8, device="cuda")
    wave = torch.full((64,), -7.0, device="cuda")
    c, w = codes.data_ptr(), wave.data_ptr()
    assert c % 16 == 0 and w % 16 == 0
    for law in GC.LAWS:
        assert L.gtcrn_g711_to_f32(0, law, c, w, 24, sp) == -1                   # n not a multiple of 16
        assert L.gtcrn_g711_to_f32(0, law, c + 1, w, 16, sp) == -1               # misaligned codes
        assert L.gtcrn_g711_to_f32(0, law, c, w + 4, 16, sp) == -1               # misaligned floats
        assert L.gtcrn_f32_to_g711(0, law, w, c, 24, sp) == -1
        assert L.gtcrn_f32_to_g711(0, law, w + 4, c, 16, sp) == -1
        assert L.gtcrn_f32_to_g711(0, law, w, c + 8, 16, sp) == -1
        assert L.gtcrn_g711_to_f32(0, law, c, w, 0, sp) == -1
    assert L.gtcrn_g711_to_f32(0, 2, c, w, 16, sp) == -1 and L.gtcrn_f32_to_g711(0, -1, w, c, 16, sp) == -1
    for bad in (lambda: g711_to_f32(codes[:24], "ulaw"), lambda: g711_to_f32(codes[1:17], "ulaw"),
                lambda: f32_to_g711(wave[1:17], "alaw"), lambda: g711_to_f32(codes, "mulaw"), lambda: f32_to_g711(wave, None),
                lambda: g711_to_f32(wave, "ulaw"), lambda: f32_to_g711(codes, "ulaw")):
        with pytest.raises(GtcrnError):
            bad()
    torch.cuda.synchronize()
    assert (wave == -7.0).all() and not codes.any()


# ---------------------------------------------------------------------------------------------- 2. the group form, bit for bit
@pytest.mark.parametrize("law,fs,n", GROUP_CASES)
def test_group_form_equals_the_float_form_through_the_pcm16_rounding(eng, win, ref, law, fs, n):
    """Three streams, 12 calls (n16 = 160: a period is 8 calls, h = 0,1,0,1,1,0,1,1; 20 ms at 8 kHz is n16 = 320, a period
    of 4): the bytes are E_law of the PCM16 rounding of the float call's output, both hand-offs are the float call's, and so
    are all three states."""
    N = 3
    codes = rand_codes(N, n * CALLS, 1000 * law + fs // 100 + n)
    xf = dec(ref, law, codes)
    A = eng.new_packet_state(N, win, n, fs, g711=GC.NAMES[law])
    B = eng.new_packet_state(N, win, n, fs)
    n16 = n * 16000 // fs
    assert A.g711 == law and B.g711 is None and A.period <= 8 < CALLS and A.n16 == n16
    hops, outs = 0, []
    for k in range(CALLS):
        a = eng.packet_stream_step(A, codes[:, n * k:n * (k + 1)].contiguous())
        b = eng.packet_stream_step(B, xf[:, n * k:n * (k + 1)].contiguous())
        assert a.dtype == torch.uint8 and tuple(a.shape) == (N, n)
        assert torch.equal(a, enc(ref, law, b)), k
        assert A.last_hops == B.last_hops
        for which in (0, 1):
            assert torch.equal(eng.packet_stream_handoff(A, which), eng.packet_stream_handoff(B, which)), (k, which)
        if hops == 0:
            # before any hop is emitted: the FIFO pre-fill and the zeros the wave step's first hop emits
            assert (a == zero_code(law)).all(), k
        hops += A.last_hops
        outs.append(a)
    assert hops == (CALLS * n16) // 256
    assert torch.equal(A.model, B.model) and torch.equal(A.wave, B.wave) and torch.equal(A.pkt, B.pkt) and A.phase == B.phase
    out = torch.cat(outs, 1)
    if fs == 16000:                                                 # the header's contract: out[k] = 0 for k < L16
        assert (out[:, :A.latency16] == zero_code(law)).all()
    assert (out != zero_code(law)).any(dim=1).all()                 # every stream emitted something
    # float32 and int16 rows stay legal on a state made with a law
    from gtcrn_micro_amd import f32_to_pcm16
    assert eng.packet_stream_step(A, xf[:, :n].contiguous()).dtype == torch.float32
    assert eng.packet_stream_step(A, f32_to_pcm16(xf[:, :n].contiguous())).dtype == torch.int16


# ---------------------------------------------------------------------------------------------- 3. the slot form
S = 5
SCHED = [[0, 1, 2], [2, 0], [], [3, 1, 4, 0], [4], [1, 2, 3], [0, 4, 2], [3], [1, 0, 4, 2, 3], [2, 3], [4, 1], [0, 3, 2]]
REJOIN = {6: [2, 4]}            # reset by the kernel before that tick: the slots start new clips mid-way


def padded(ids, n=S):
    return i32(list(ids) + [s for s in range(n) if s not in ids])


def four(st):
    return [t.clone() for t in (st.model, st.wave, st.pkt, st.phase)]


def float_truth(eng, win, ref, law, fs, n, packets):
    """A one-stream FLOAT group created fresh, fed D[c] / 32768 of `packets` (k, n): (E_law of its PCM16 output, state)."""
    st = eng.new_packet_state(1, win, n, fs)
    outs = [enc(ref, law, eng.packet_stream_step(st, dec(ref, law, packets[k:k + 1]))) for k in range(packets.shape[0])]
    return (torch.cat(outs, 1)[0] if outs else packets.new_zeros(0)), st


@pytest.mark.parametrize("law,fs,n", [(0, 8000, 160), (1, 8000, 80)])
def test_slot_form_ragged_schedule_and_a_join(eng, win, ref, law, fs, n):
    assert len(SCHED) == CALLS and [] in SCHED and any(t != sorted(t) for t in SCHED)
    codes = rand_codes(S, n * CALLS, 77 + law)
    st = eng.new_packet_slot_state(S, win, n, fs, g711=GC.NAMES[law])
    seen, first = [0] * S, [0] * S
    blocks = [[] for _ in range(S)]
    xin = torch.zeros((S, n), dtype=torch.uint8, device="cuda")
    out = torch.empty((S, n), dtype=torch.uint8, device="cuda")
    for t, ids in enumerate(SCHED):
        for s in REJOIN.get(t, []):
            assert seen[s] > 0 and int(st.phase[s]) != 0                         # it leaves mid-hop
            b0 = four(st)
            eng.packet_stream_reset_slots(st, i32([s]))
            others = [r for r in range(S) if r != s]
            assert all(torch.equal(a[others], b[others]) and not a[s].any() for a, b in zip(four(st), b0))
            first[s], blocks[s] = seen[s], []
        xin.zero_()
        for i, s in enumerate(ids):
            xin[i] = codes[s, n * seen[s]:n * (seen[s] + 1)]
        out.fill_(0xAA)
        b0 = four(st)
        eng.packet_stream_step_slots(st, padded(ids), xin, count=i32([len(ids)]), out=out)
        assert (out[len(ids):] == 0xAA).all(), t                                 # rows at or beyond the count: not written
        idle = [s for s in range(S) if s not in ids]
        assert all(torch.equal(a[idle], b[idle]) for a, b in zip(four(st), b0)), t   # slots not named: untouched
        for i, s in enumerate(ids):
            blocks[s].append(out[i].clone())
            seen[s] += 1
    for s in range(S):
        assert seen[s] - first[s] >= 3
        pk = codes[s, n * first[s]:n * seen[s]].reshape(seen[s] - first[s], n)
        want, ts = float_truth(eng, win, ref, law, fs, n, pk)
        assert torch.equal(torch.cat(blocks[s]), want), s
        assert torch.equal(st.model[s:s + 1], ts.model) and torch.equal(st.wave[s:s + 1], ts.wave), s
        assert torch.equal(st.pkt[s:s + 1], ts.pkt) and int(st.phase[s]) == ts.phase, s
    assert len(set(st.phase.tolist())) > 1
    assert any((torch.cat(b) != zero_code(law)).any() for b in blocks)


# ---------------------------------------------------------------------------------------------- 4. gains and meters compose
@pytest.mark.parametrize("law,fs,n", [(0, 16000, 160), (1, 16000, 160), (1, 8000, 160), (0, 8000, 80)])
def test_gains_and_meters_compose(eng, win, ref, law, fs, n):
    """Streams limited to 0 dB (bypass), 12 dB and not at all, with meters: the bytes are E_law of the PCM16 rounding of the
    float-input limited run and the meter records are that run's, bit for bit (mix and meters are taken in float at 16 kHz,
    before the encode).  At 16 kHz the bypassed stream returns E(D[c]) per code, L16 samples late."""
    N, db = 3, [0.0, 12.0, None]
    codes = rand_codes(N, n * CALLS, 31 + 7 * law + n)
    xf = dec(ref, law, codes)
    A = eng.new_packet_state(N, win, n, fs, atten_lim_db=db, meters=True, g711=GC.NAMES[law])
    B = eng.new_packet_state(N, win, n, fs, atten_lim_db=db, meters=True)
    assert A.dry_gain.tolist() == B.dry_gain.tolist() and A.dry_gain[0] == 1.0 and A.dry_gain[2] == 0.0
    outs = []
    for k in range(CALLS):
        a = eng.packet_stream_step(A, codes[:, n * k:n * (k + 1)].contiguous())
        b = eng.packet_stream_step(B, xf[:, n * k:n * (k + 1)].contiguous())
        assert torch.equal(a, enc(ref, law, b)), k
        assert torch.equal(A.meters.view(torch.int32), B.meters.view(torch.int32)), k
        outs.append(a)
    assert (A.meters[:, 3] == (CALLS * n * 16000 // fs) // 256).all() and (A.meters[:, :3] > 0).all()
    out = torch.cat(outs, 1)
    assert not torch.equal(out[1], out[0]) and (out[2] != zero_code(law)).any()
    if fs == 16000:
        L16 = A.latency16
        assert L16 == 512 - gcd(n, 256)
        D, _, E = ref[law]
        assert (out[0, :L16] == zero_code(law)).all()
        assert torch.equal(out[0, L16:], E[D[codes[0, :n * CALLS - L16].long()] + 32768])
        if law == 1:                                                  # A-law has no double zero: the codes themselves
            assert torch.equal(out[0, L16:], codes[0, :n * CALLS - L16])


# ---------------------------------------------------------------------------------------------- 5. one capture serves
def test_one_captured_slot_call_serves_every_tick(eng, win, ref):
    """ONE capture of ONE G.711 slot call (8 kHz, 20 ms mu-law), replayed over 8 ticks (a whole period) with the table, the
    count and the input bytes rewritten between replays, equals the eager run."""
    law, fs, n, M = 0, 8000, 160, 4
    codes = rand_codes(S, n * 8, 99)
    rng = np.random.default_rng(8)
    ticks = [(rng.permutation(S)[:M], c) for c in [4, 0, 2, 4, 1, 3, 4, 2]]
    seen, inputs = [0] * S, []
    for perm, c in ticks:
        x = torch.zeros((M, n), dtype=torch.uint8, device="cuda")
        for i in range(c):
            s = int(perm[i])
            x[i] = codes[s, n * seen[s]:n * (seen[s] + 1)]
            seen[s] += 1
        inputs.append(x)

    def fresh():
        return eng.new_packet_slot_state(S, win, n, fs, max_active=M, g711="ulaw")

    se = fresh()
    eager = [eng.packet_stream_step_slots(se, i32(p), x, count=i32([c])).clone()[:c] for (p, c), x in zip(ticks, inputs)]
    assert len(set(se.phase.tolist())) > 1 and any((e != 0xFF).any() for e in eager)
    sg = fresh()
    slots, count = i32(ticks[0][0]), i32([0])
    xin = torch.zeros((M, n), dtype=torch.uint8, device="cuda")
    out = torch.zeros((M, n), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.packet_stream_step_slots(sg, slots, xin, count=count, out=out)        # warm-up with count 0: nothing steps
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.packet_stream_step_slots(sg, slots, xin, count=count, out=out)
    for k, ((p, c), xk) in enumerate(zip(ticks, inputs)):
        slots.copy_(i32(p))
        count.fill_(c)
        xin.copy_(xk)
        graph.replay()
        assert torch.equal(out[:c], eager[k]), k
    assert all(torch.equal(a, b) for a, b in zip(four(sg), four(se)))


# ---------------------------------------------------------------------------------------------- 6. launch sequence
def _launches(eng, fn):
    eng.timing_enable(True)
    fn()
    torch.cuda.synchronize()
    t = {k: v[1] for k, v in eng.timing_read().items()}
    eng.timing_enable(False)
    return t


@pytest.mark.parametrize("law,fs,n", [(0, 8000, 80), (1, 16000, 160)])
def test_a_g711_call_makes_the_float_calls_launches(eng, win, ref, law, fs, n):
    """From the library's launch records, over a whole period of phases: the same kernels the same number of times as the
    float call at the same (fs, n, phase) -- contiguous form and slot form."""
    codes = rand_codes(S, n * 8, 5)
    xf = dec(ref, law, codes)
    A, B = eng.new_packet_state(S, win, n, fs, g711=GC.NAMES[law]), eng.new_packet_state(S, win, n, fs)
    hs = []
    for k in range(8):
        ck, fk = codes[:, n * k:n * (k + 1)].contiguous(), xf[:, n * k:n * (k + 1)].contiguous()
        assert A.phase == B.phase
        la, lb = _launches(eng, lambda: eng.packet_stream_step(A, ck)), _launches(eng, lambda: eng.packet_stream_step(B, fk))
        assert la == lb and la["k_packet_in"] == 1 and la["k_packet_out"] == 1, (k, la, lb)
        hs.append(A.last_hops)
    assert hs == [0, 1, 0, 1, 1, 0, 1, 1]
    SA, SB = eng.new_packet_slot_state(S, win, n, fs, g711=GC.NAMES[law]), eng.new_packet_slot_state(S, win, n, fs)
    for k, ids in enumerate(SCHED[:8]):
        ck, fk = codes[:, n * k:n * (k + 1)].contiguous(), xf[:, n * k:n * (k + 1)].contiguous()
        cnt = i32([len(ids)])
        la = _launches(eng, lambda: eng.packet_stream_step_slots(SA, padded(ids), ck, count=cnt))
        lb = _launches(eng, lambda: eng.packet_stream_step_slots(SB, padded(ids), fk, count=cnt))
        assert la == lb and la["k_packet_plan"] == 1 and la["k_packet_in_slots"] == 1 and la["k_packet_out_slots"] == 1, (k, la)
    assert torch.equal(SA.phase, SB.phase) and torch.equal(SA.pkt, SB.pkt)


# ---------------------------------------------------------------------------------------------- 7. errors leave states alone
def test_error_paths_leave_states_and_outputs_alone(eng, win):
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import lib
    fs, n, N, M = 8000, 160, 3, 4
    L, sp = lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    codes = rand_codes(S, 2 * n, 3)
    # the contiguous form
    G = eng.new_packet_state(N, win, n, fs, g711="ulaw")
    eng.packet_stream_step(G, codes[:N, :n].contiguous())
    eng.packet_stream_step(G, codes[:N, n:].contiguous())
    g0, gphase = [t.clone() for t in (G.model, G.wave, G.pkt)], G.phase
    xin = codes[:N, :n].contiguous()
    out = torch.full((S, n), 0xAA, dtype=torch.uint8, device="cuda")
    m, w, p, xi, o, wi = (G.model.data_ptr(), G.wave.data_ptr(), G.pkt.data_ptr(), xin.data_ptr(), out.data_ptr(),
                          G.window.data_ptr())
    step = L.gtcrn_packet_stream_step_g711
    calls = [
        lambda: step(G._h, m, w, p, xi, n, o, n, N, 2, wi, sp),                 # law outside {0, 1}
        lambda: step(G._h, m, w, p, xi, n, o, n, N, -1, wi, sp),
        lambda: step(None, m, w, p, xi, n, o, n, N, 0, wi, sp),                 # null pointers
        lambda: step(G._h, None, w, p, xi, n, o, n, N, 0, wi, sp),
        lambda: step(G._h, m, w, None, xi, n, o, n, N, 0, wi, sp),
        lambda: step(G._h, m, w, p, None, n, o, n, N, 0, wi, sp),
        lambda: step(G._h, m, w, p, xi, n, None, n, N, 1, wi, sp),
        lambda: step(G._h, m, w, p, xi, n, o, n, N, 1, None, sp),
        lambda: step(G._h, m, w, p, xi, n - 1, o, n, N, 0, wi, sp),             # a stride < n
        lambda: step(G._h, m, w, p, xi, n, o, n - 1, N, 1, wi, sp),
        lambda: step(G._h, m, w, p, xi, n, o, n, N + 1, 0, wi, sp),             # more streams than the handle's
        lambda: step(G._h, m, w, p, xi, n, o, n, 0, 0, wi, sp),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i                                                      # GTCRN_ERR_ARG
        assert L.gtcrn_last_error(), i
    torch.cuda.synchronize()
    assert (out == 0xAA).all() and G.phase == gphase
    assert all(torch.equal(a, b) for a, b in zip((G.model, G.wave, G.pkt), g0))
    # the slot form
    st = eng.new_packet_slot_state(S, win, n, fs, max_active=M, g711="alaw")
    good = i32([3, 0, 4, 1])
    eng.packet_stream_step_slots(st, good, codes[[3, 0, 4, 1], :n].contiguous())
    b0 = four(st)
    hop = codes[:M, n:].contiguous()
    m, w, p, ph, sl, xi, wi = (st.model.data_ptr(), st.wave.data_ptr(), st.pkt.data_ptr(), st.phase.data_ptr(),
                               good.data_ptr(), hop.data_ptr(), st.window.data_ptr())
    step = L.gtcrn_packet_stream_step_slots_g711
    calls = [
        lambda: step(st._h, m, w, p, ph, sl, None, M, xi, n, o, n, 2, wi, sp),           # law
        lambda: step(st._h, m, w, p, ph, sl, None, M, xi, n, o, n, 256, wi, sp),
        lambda: step(None, m, w, p, ph, sl, None, M, xi, n, o, n, 1, wi, sp),            # null pointers
        lambda: step(st._h, m, w, p, None, sl, None, M, xi, n, o, n, 1, wi, sp),
        lambda: step(st._h, m, w, p, ph, None, None, M, xi, n, o, n, 1, wi, sp),
        lambda: step(st._h, m, w, p, ph, sl, None, M, None, n, o, n, 1, wi, sp),
        lambda: step(st._h, m, w, p, ph, sl, None, M, xi, n, None, n, 0, wi, sp),
        lambda: step(st._h, m, w, p, ph, sl, None, M, xi, n - 1, o, n, 1, wi, sp),       # a stride < n
        lambda: step(st._h, m, w, p, ph, sl, None, M, xi, n, o, n - 1, 0, wi, sp),
        lambda: step(st._h, m, w, p, ph, sl, None, M + 1, xi, n, o, n, 1, wi, sp),       # max_active above the handle's
        lambda: step(st._h, m, w, p, ph, sl, None, 0, xi, n, o, n, 1, wi, sp),
        lambda: step(st._h, m, w, p + 4, ph, sl, None, M, xi, n, o, n, 1, wi, sp),       # a state off the 16-byte grid
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i
        assert L.gtcrn_last_error(), i
    # the Python layer: uint8 needs the law; other dtypes and shapes are refused as before
    lawless, lawless_slots = eng.new_packet_state(N, win, n, fs), eng.new_packet_slot_state(S, win, n, fs, max_active=M)
    bad = [
        lambda: eng.packet_stream_step(lawless, xin),
        lambda: eng.packet_stream_step_slots(lawless_slots, good, hop),
        lambda: eng.packet_stream_step(G, xin[:, :80].contiguous()),
        lambda: eng.packet_stream_step(G, xin.to(torch.int8)),
        lambda: eng.packet_stream_step_slots(st, good, hop, out=out[:M].to(torch.int16)),
        lambda: eng.new_packet_state(N, win, n, fs, g711="mulaw"),
        lambda: eng.new_packet_slot_state(S, win, n, fs, g711=2),
        lambda: eng.wave_stream_step(eng.new_wave_state(N, win), torch.zeros((N, 256), dtype=torch.uint8, device="cuda")),
    ]
    for i, c in enumerate(bad):
        with pytest.raises(GtcrnError):
            c()
    torch.cuda.synchronize()
    assert (out == 0xAA).all()
    assert all(torch.equal(a, b) for a, b in zip(four(st), b0))
    assert all(torch.equal(a, b) for a, b in zip((G.model, G.wave, G.pkt), g0)) and G.phase == gphase
    assert not lawless.pkt.any() and lawless.phase == 0 and not lawless_slots.pkt.any() and not lawless_slots.phase.any()


def test_streaming_wrapper_takes_the_law(win, ref):
    """The 8 kHz PCMU example of INTEGRATION.md: fs=8000, packet=160, g711="ulaw"."""
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import PacketSlotState, PacketStreamState
    from gtcrn_micro_amd.streaming.gtcrn_micro_stream import StreamGTCRNMicro
    stream = StreamGTCRNMicro().cuda().eval()
    n = 160
    codes = rand_codes(2, n * 4, 41)
    st = stream.init_wave_state(2, win, fs=8000, packet=n, g711="ulaw")
    assert isinstance(st, PacketStreamState) and st.g711 == 0 and st.n16 == 320
    e = stream.engine(codes.device)
    truth = e.new_packet_state(2, win, n, 8000)
    for k in range(4):
        pk = codes[:, n * k:n * (k + 1)].contiguous()
        got = stream.step_wave(pk, st)
        assert got.dtype == torch.uint8 and torch.equal(got, enc(ref, 0, e.packet_stream_step(truth, dec(ref, 0, pk)))), k
    rs = stream.init_wave_state(3, win, fs=8000, packet=n, resident=True, g711="alaw")
    assert isinstance(rs, PacketSlotState) and rs.g711 == 1
    assert stream.step_wave(codes[:, :n].contiguous(), rs, slots=i32([2, 0])).dtype == torch.uint8
    with pytest.raises(GtcrnError):
        stream.init_wave_state(2, win, fs=8000, g711="ulaw")                      # the rate form takes no codes
    with pytest.raises(GtcrnError):
        stream.step_wave(codes[:, :n].contiguous(), stream.init_wave_state(2, win, fs=8000, packet=n))
