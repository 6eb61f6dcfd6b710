"""Isolation of streams: one non-finite element in ONE stream, utterance or row changes no bit of another, and the victim
heals by itself.  Every form of the library runs twice on the same seeded input -- clean, and with one element of one victim
replaced by a quiet NaN, +Inf or 1e30 -- and the two runs are compared bit for bit (isolation_checker.same_bits):

  P1 isolation   every other stream's outputs, at every call, and its rows of every state tensor at the end
  P2 causality   the victim's outputs before the poisoned call
  P3 cone        (NaN only) the victim's non-finite outputs are exactly the float64 reference's: 85 frames, every bin, at
                 spectrum level; 87 blocks of 256 samples, every sample, at wave level (tests/test_isolation_host.py pins
                 both on the CPU; no number here comes from a GPU run)
  P4 recovery    the victim's outputs after the cone, and its whole state at the end of a run that goes on for CONE + RING
                 frames after the poison: no field of the state accumulates
  P5 reset cure  a third run resets the victim alone two frames into the cone, through the form's own reset: from then on
                 its outputs and state are those of a fresh stream fed the same samples

A finite test cannot see any of this: 0 * x == 0 hides a value that crossed from one stream into another and was masked by a
multiply; 0 * NaN does not.  No tolerance appears below.

The poison sits where the window is not zero and no edge reflection reaches: sample index not a multiple of 256, >= 257 and
more than 512 from the end (but for the dedicated end-of-clip case).  A NaN at exactly sample 256 legitimately differs
between the offline and the live forms -- the hop form frames hop 0 without its future sample x[256], which meets
win[0] == 0, while the offline frame 0 (torch.stft's reflected one) reads it -- and is not tested.

Not covered, by definition: training (train-mode BatchNorm and the batch-mean loss couple the clips of a batch), and the
integer sample forms (PCM16, G.711), which cannot carry the poison in."""
from math import gcd

import numpy as np
import pytest

import isolation_checker as IC
import resample_checker as RC
from conftest import load_params

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CONE, RING = IC.CONE, IC.RING
KINDS = ["nan", "inf", "1e30"]
T, T0 = 112, 7                       # spectrum level: frames per run, the poisoned frame
assert T - T0 >= CONE + RING
BIN = 200                            # the poisoned element: re of this bin


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
    e.var_spans_enable(True)


@pytest.fixture(scope="module")
def win(dev):
    return torch.hann_window(512).pow(0.5).cuda()


def i32(ids):
    return torch.tensor(list(ids), dtype=torch.int32, device="cuda")


def noise(shape, seed, amp):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=gen) * amp


def poisoned(x, index, kind):
    y = x.clone()
    y[index] = IC.POISONS[kind]
    return y


def same(a, b, what):
    """assert same_bits(a, b), naming the first element that differs."""
    if IC.same_bits(a, b):
        return
    a, b = IC._np(a), IC._np(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(IC._bits(a) != IC._bits(b))
    raise AssertionError(f"{what}: {len(bad)} of {a.size} elements differ, first at {tuple(bad[0])}: "
                         f"{a[tuple(bad[0])]!r} != {b[tuple(bad[0])]!r}")


def snap(st, meters=False, hb=False):
    """Every state tensor of a state object (or the bare model state of stream_step), copied to the host.  The tensors are
    named by the state's type -- model and wave; rate for a rate state; pkt and phase for a packet state; meters and hb where
    the caller made the state with them -- and read as attributes, so that a tensor the library renames or drops fails here
    instead of shrinking the comparison."""
    from gtcrn_micro_amd._lib import PacketSlotState, PacketStreamState, RateStreamState, WaveStreamState
    if isinstance(st, torch.Tensor):
        return {"model": st.cpu().numpy()}
    assert isinstance(st, WaveStreamState), type(st)
    out = {"model": st.model, "wave": st.wave}
    if isinstance(st, RateStreamState):
        out["rate"] = st.rate
    if isinstance(st, PacketStreamState):
        out["pkt"] = st.pkt
        if isinstance(st, PacketSlotState):
            out["phase"] = st.phase
        else:
            assert isinstance(st.phase, int), type(st.phase)
            out["phase"] = torch.tensor([st.phase], dtype=torch.int32)   # (the group's host phase: one word for all streams)
    if meters:
        out["meters"] = st.meters
    else:
        assert st.meters is None
    if hb:
        out["hb"] = st.hb
    else:
        assert getattr(st, "hb", None) is None
    for name, t in out.items():
        assert isinstance(t, torch.Tensor) and t.shape[0] in (st.n, 1), (name, type(t))
    return {name: t.cpu().numpy() for name, t in out.items()}


def same_states(a, b, rows_a, rows_b, what):
    """Rows rows_a of every tensor of snapshot a == rows rows_b of snapshot b, and the two hold the same tensors."""
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for name in a:
        if a[name].shape[0] == 1 and name == "phase":
            same(a[name], b[name], f"{what}: state.{name}")
        else:
            same(a[name][rows_a], b[name][rows_b], f"{what}: state.{name} rows {rows_a}")


def others(n, v):
    return [i for i in range(n) if i != v]


def check_frames(clean, bad, v, t0, kind, what, p3=True):
    """P1..P4 on spectrum outputs (N,257,T,2): the victim v was poisoned in frame t0."""
    n, nt = clean.shape[0], clean.shape[2]
    clean, bad = IC._np(clean), IC._np(bad)
    end = min(t0 + CONE, nt)
    same(bad[others(n, v)], clean[others(n, v)], f"{what}: P1 other rows")
    same(bad[v][:, :t0], clean[v][:, :t0], f"{what}: P2 frames before {t0}")
    same(bad[v][:, end:], clean[v][:, end:], f"{what}: P4 frames from {end}")
    if kind == "nan" and p3:
        got = IC.nonfinite_frames(bad[v], axis=1)
        assert got == {t: True for t in IC.cone_frames(t0, nt)}, \
            (what, "P3", sorted(got), [t for t, full in got.items() if not full])


def check_blocks(clean, bad, v, cone, kind, what, p3=True):
    """P1..P4 on waveform outputs (N, 256 K): `cone` is the set of 256-sample blocks the reference makes non-finite."""
    n = clean.shape[0]
    clean, bad = IC._np(clean), IC._np(bad)
    lo, hi = 256 * min(cone), 256 * (max(cone) + 1)
    same(bad[others(n, v)], clean[others(n, v)], f"{what}: P1 other rows")
    same(bad[v][:lo], clean[v][:lo], f"{what}: P2 blocks before {min(cone)}")
    same(bad[v][hi:], clean[v][hi:], f"{what}: P4 blocks after {max(cone)}")
    if kind == "nan" and p3:
        got = IC.nonfinite_frames(bad[v], block=256)
        assert got == {b: True for b in cone}, (what, "P3", sorted(got), [b for b, full in got.items() if not full])


def check_run_of_samples(clean, bad, v, start, clean_from, min_run, kind, what):
    """P1..P4 where the resampling filters blur the cone's edges (rate and packet forms): the victim's non-finite outputs
    are one contiguous run that starts no earlier than sample `start`, and from sample `clean_from` on the bits are the clean
    run's.  The run is no shorter than `min_run` samples: the reference's cone less its blurred edges."""
    n = clean.shape[0]
    clean, bad = IC._np(clean), IC._np(bad)
    same(bad[others(n, v)], clean[others(n, v)], f"{what}: P1 other rows")
    same(bad[v][:start], clean[v][:start], f"{what}: P2 samples before {start}")
    same(bad[v][clean_from:], clean[v][clean_from:], f"{what}: P4 samples from {clean_from}")
    if kind == "nan":
        idx = np.flatnonzero(~np.isfinite(bad[v]))
        assert idx.size and idx[0] >= start and idx[-1] - idx[0] + 1 == idx.size, (what, "P3", idx[:1], idx[-1:], idx.size)
        assert idx.size >= min_run, (what, "P3", idx.size, min_run)


def drive(step, x, unit, calls, before=None):
    """x (N, unit K) through step() in calls of `calls` units; before = {unit index: callable}, run ahead of the call that
    starts there.  Returns the outputs side by side."""
    outs, k = [], 0
    for n in calls:
        if before and k in before:
            before[k]()
        outs.append(step(x[:, unit * k:unit * (k + n)]).clone())
        k += n
    assert unit * k == x.shape[1]
    return torch.cat(outs, 1)


def calls_from(calls, k0):
    """The calls of a schedule that start at unit k0 or later (k0 must be a call boundary)."""
    k = 0
    for i, n in enumerate(calls):
        if k == k0:
            return calls[i:]
        k += n
    raise AssertionError(f"{k0} is no call boundary")


# ---- spectrum streaming: stream_step, frame by frame and in chunks -----------------------------------------------------------
def reset_model_rows(eng, st, v):
    """gtcrn_stream_reset on stream v alone (new_state runs it on all rows)."""
    eng.stream_reset(st, v, v + 1)


def run_frames(eng, form, x, chunks, reset=None):
    """x (N,257,T,2) through stream_step in calls of `chunks` frames under stream_form(form); reset = (frame, stream): that
    stream alone is reset ahead of the call that starts at that frame.  Returns (outputs, state snapshot)."""
    eng.stream_form(form)
    try:
        st = eng.new_state(x.shape[0])
        outs, t = [], 0
        for n in chunks:
            if reset and reset[0] == t:
                reset_model_rows(eng, st, reset[1])
            outs.append(eng.stream_step(st, x[:, :, t:t + n]))
            t += n
        assert t == x.shape[2]
        return torch.cat(outs, 2).cpu().numpy(), snap(st)
    finally:
        eng.stream_form(0)


FORMS = {2: (9, [0, 1, 3, 4, 8]),          # four streams per workgroup: two full workgroups and a lone stream
         3: (15, [0, 3, 6, 7, 14]),        # seven per workgroup: two full ones and a lone stream
         1: (5, [0, 2, 4])}                # three launches: the GTCN tiles straddle streams
SINGLE = [1] * T
CHUNKS = [1, 4, 16, 17, 2, 33, 39]
assert sum(CHUNKS) == T


@pytest.fixture(scope="module")
def spectra():
    return noise((15, IC.NBINS, T, 2), 85, 0.3)


_FRAME_RUNS = {}


def frame_run(eng, spectra, form, n, chunks, v=None, kind=None, t0=T0):
    """The (cached) clean run of a form, or its run with stream v poisoned."""
    key = (form, n, tuple(chunks), v, kind, t0)
    if key not in _FRAME_RUNS:
        x = spectra[:n]
        if v is not None:
            x = poisoned(x, (v, BIN, t0, 0), kind)
        _FRAME_RUNS[key] = run_frames(eng, form, x, chunks)
    return _FRAME_RUNS[key]


def frame_case(eng, spectra, form, n, chunks, v, kind, t0, reset_at):
    what = f"stream_form({form}) N={n} victim {v} {kind}"
    clean, cst = frame_run(eng, spectra, form, n, chunks)
    bad, bst = frame_run(eng, spectra, form, n, chunks, v, kind, t0)
    check_frames(clean, bad, v, t0, kind, what)
    same_states(bst, cst, slice(None), slice(None), f"{what}: P1 + P4 at the end")
    # P5: the victim alone is reset inside the cone; a fresh stream fed the frames from there on is the truth
    xb = poisoned(spectra[:n], (v, BIN, t0, 0), kind)
    cured, ust = run_frames(eng, form, xb, chunks, reset=(reset_at, v))
    fresh, fst = run_frames(eng, form, xb[v:v + 1, :, reset_at:].contiguous(), calls_from(chunks, reset_at))
    same(cured[v][:, reset_at:], fresh[0], f"{what}: P5 outputs after the reset")
    same_states(ust, fst, slice(v, v + 1), slice(0, 1), f"{what}: P5")
    same(cured[others(n, v)], clean[others(n, v)], f"{what}: P5 leaves the other rows alone")
    same_states(ust, cst, others(n, v), others(n, v), f"{what}: P5 leaves the other rows alone")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form,v", [(f, v) for f, (_, vs) in FORMS.items() for v in vs])
def test_stream_step_frame_by_frame(eng, spectra, form, v, kind):
    frame_case(eng, spectra, form, FORMS[form][0], SINGLE, v, kind, T0, T0 + 2)


@pytest.mark.parametrize("kind", KINDS)
def test_stream_step_forms_agree_on_the_victim(eng, spectra, kind):
    """Stream 0 sees the same frames in all three forms: its outputs agree wherever they are not both non-finite, and its
    healed state is one and the same, as test_single_launch_step_equals_the_three_launch_form states for clean input."""
    runs = {f: frame_run(eng, spectra, f, FORMS[f][0], SINGLE, 0, kind) for f in FORMS}
    for f in (2, 3):
        assert IC.same_bits_or_both_nonfinite(runs[f][0][0], runs[1][0][0]), (f, kind)
        same_states(runs[f][1], runs[1][1], slice(0, 1), slice(0, 1), f"form {f} vs three launches, {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_stream_step_in_chunks(eng, spectra, kind):
    """Calls of 1, 4, 16, 17, 2, 33 and 39 frames; the poison inside the 16-frame call (frames 5 .. 20).  The reset of P5 falls
    on the next call boundary."""
    t0 = 10
    assert 5 < t0 < 20 and T - t0 >= CONE + RING
    frame_case(eng, spectra, 0, 5, CHUNKS, 2, kind, t0, 21)


@pytest.mark.parametrize("kind", KINDS)
def test_stream_step_slots(eng, spectra, kind):
    """8 resident streams; every call names slots 6, 1, 3, 0 and, beyond the device count of 4, slot 5, whose input row is NaN
    in every call.  The victim is slot 3.  Slots 2, 4, 7 and 5 keep the bits of a state that was never stepped."""
    table, count = i32([6, 1, 3, 0, 5]), i32([4])
    named, idle, v, row = [6, 1, 3, 0], [2, 4, 5, 7], 3, 2
    what = f"stream_step_slots {kind}"

    def run(x, reset_at=None):
        st = eng.new_state(8)
        eng.stream_step(st, spectra[:8, :, :3].flip(0).contiguous())            # every slot holds history
        before = snap(st)
        outs = []
        for t in range(T):
            if reset_at == t:
                reset_model_rows(eng, st, v)
            xin = torch.full((5, IC.NBINS, 1, 2), IC.QNAN, device="cuda")
            xin[:4] = x[named, :, t:t + 1]
            out = torch.full((5, IC.NBINS, 1, 2), -7.0, device="cuda")
            eng.stream_step_slots(st, table, xin, count=count, out=out)
            outs.append(out)
        return torch.cat(outs, 2).cpu().numpy(), snap(st), before

    x = spectra[:8]
    clean, cst, before = run(x)
    assert (clean[4] == -7.0).all() and np.isfinite(clean[:4]).all()
    same_states(cst, before, idle, idle, f"{what}: idle slots (clean run)")
    xb = poisoned(x, (v, BIN, T0, 0), kind)
    bad, bst, _ = run(xb)
    check_frames(clean, bad, row, T0, kind, what)
    same_states(bst, before, idle, idle, f"{what}: P1 idle slots")
    same_states(bst, cst, slice(None), slice(None), f"{what}: P1 + P4 at the end")
    cured, ust, _ = run(xb, reset_at=T0 + 2)
    fresh, fst = run_frames(eng, 0, xb[v:v + 1, :, T0 + 2:].contiguous(), [1] * (T - T0 - 2))
    same(cured[row][:, T0 + 2:], fresh[0], f"{what}: P5 outputs after the reset")
    same_states(ust, fst, slice(v, v + 1), slice(0, 1), f"{what}: P5")
    same_states(ust, cst, others(8, v), others(8, v), f"{what}: P5 leaves the other slots alone")


# ---- offline, spectrum level ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nt,v,t0", [(T, 1, T0), (T, 1, 109), (T - 1, 0, 108), (T - 1, 1, 108)])
def test_forward_spec(eng, spectra, kind, nt, v, t0):
    """B = 3 runs in time spans: 256 workgroups take equal shares of the flattened (utterance, frame) axis.  With the cone at
    the end of its utterance it abuts the next one's first frames, which start from zero history and not from the victim's
    last frames.  T = 112 is a multiple of the two-frame share, so there every share lies inside one utterance; at T = 111 the
    share that holds utterance 0's last frame runs on into utterance 1 in the same workgroup, over rings it has to clear."""
    x = spectra[:3, :, :nt].contiguous()
    clean = eng.forward_spec(x)
    bad = eng.forward_spec(poisoned(x, (v, BIN, t0, 0), kind))
    check_frames(clean, bad, v, t0, kind, f"forward_spec T={nt} victim {v} t0={t0} {kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("v", [255, 256])
def test_forward_spec_many_utterances(eng, kind, v):
    """B = 257, T = 20: 256 workgroups and then spans; the victim is the last utterance of the first round and the lone one."""
    x = noise((257, IC.NBINS, 20, 2), 257, 0.3)
    clean = eng.forward_spec(x)
    bad = eng.forward_spec(poisoned(x, (v, BIN, 18, 0), kind))
    check_frames(clean, bad, v, 18, kind, f"forward_spec B=257 victim {v} {kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scales", ["fp16", "int8"])
def test_forward_spec_quant(eng, spectra, kind, scales):
    """The int8 / fp16 variant: P1, P2 and P4 (its int8 boundary may clip the poison away, so no P3)."""
    from oracle.quant_port import CALIB_SCALE
    sc = (0.0, 0.0) if scales == "fp16" else (CALIB_SCALE, CALIB_SCALE * 2 ** 0.5)
    x = spectra[:3]
    clean = eng.forward_spec_quant(x, *sc)
    bad = eng.forward_spec_quant(poisoned(x, (1, BIN, T0, 0), kind), *sc)
    check_frames(clean, bad, 1, T0, kind, f"forward_spec_quant {scales} {kind}", p3=False)


# ---- offline, wave level ----------------------------------------------------------------------------------------------------
HOPS = 110
SAMPLE = 256 * 9 + 100               # inside hop 9


@pytest.fixture(scope="module")
def waves():
    return noise((3, 256 * HOPS), 87, 0.1)


LATE = 256 * 107 + 100               # inside hop 107: 668 samples from the end, and the cone runs to the clip's last frame
assert IC.cone_blocks(9, HOPS) == set(range(8, 95)) and IC.cone_blocks(107, HOPS) == {106, 107, 108, 109}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("v,sample", [(1, SAMPLE), (0, LATE)])
@pytest.mark.parametrize("gains", [None, [0.25, 0.5, 0.75]])
def test_forward_wave(eng, win, waves, kind, gains, v, sample):
    """B = 3 clips of 110 hops (111 frames: a share of the time spans runs from clip 0's last frame on into clip 1), the
    poison in hop 9 of clip 1: blocks 8 .. 94; and in hop 107 of clip 0, whose cone ends where clip 1 starts in the same
    workgroup.  With per-clip dry gains the dry path adds the poisoned sample itself, which lies inside the cone: it has no
    memory."""
    g = None if gains is None else torch.tensor(gains, device="cuda")
    clean = eng.forward_wave(waves, win, dry_gain=g)
    bad = eng.forward_wave(poisoned(waves, (v, sample), kind), win, dry_gain=g)
    check_blocks(clean, bad, v, IC.cone_blocks(sample // 256, HOPS), kind, f"forward_wave gains={gains} clip {v} {kind}")


LENGTHS = [257, 256 * HOPS, 257, 256 * 30 + 17, 4097]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sample", [SAMPLE, 256 * 109 + 100])
@pytest.mark.parametrize("spans", [True, False])
def test_forward_wave_var(eng, win, waves, spans, sample, kind):
    """Clips of 257, 28160, 257, 7697 and 4097 samples in one call, the padding of every row NaN; the victim is the long clip
    between the two 257-sample ones, poisoned in hop 9 and, the one case at the end of a clip, in its last hop.  Every clip's
    own samples are compared; what lies behind them is unspecified."""
    lmax = max(LENGTHS)
    x = torch.full((5, lmax), IC.QNAN, device="cuda")
    src = noise((5, lmax), 88, 0.1)
    for b, n in enumerate(LENGTHS):
        x[b, :n] = src[b, :n]
    x[1] = waves[1]
    eng.var_spans_enable(spans)
    try:
        clean = eng.forward_wave_var(x, LENGTHS, win).cpu().numpy()
        bad = eng.forward_wave_var(poisoned(x, (1, sample), kind), LENGTHS, win).cpu().numpy()
    finally:
        eng.var_spans_enable(True)
    what = f"forward_wave_var spans={spans} sample {sample} {kind}"
    for b, n in enumerate(LENGTHS):
        m = 256 * (n // 256)
        assert np.isfinite(clean[b, :m]).all(), (what, b)                    # (the NaN padding reaches no clip)
        if b != 1:
            same(bad[b, :m], clean[b, :m], f"{what}: P1 clip {b}")
    same(clean[1], eng.forward_wave(waves[1:2], win)[0], f"{what}: the long clip alone")
    cone = IC.cone_blocks(sample // 256, HOPS)
    check_blocks(clean[1:2], bad[1:2], 0, cone, kind, what)


# ---- hop form: wave_stream_step ------------------------------------------------------------------------------------------------
LIVE_HOPS = 112
LIVE_CALLS = [1, 2, 5] * 14
H0 = 7                               # the poisoned hop: inside the call of hops 3 .. 7; hop 9 starts a call
LIVE_SAMPLE = 256 * H0 + 100
LIVE_CONE = {b + 1 for b in IC.cone_blocks(H0, LIVE_HOPS + 1)}       # one hop late
METER_RESET = 96                     # a call boundary behind the cone
assert sum(LIVE_CALLS) == LIVE_HOPS and max(LIVE_CONE) == H0 + CONE + 1 < METER_RESET
assert LIVE_HOPS - 1 >= H0 + 1 + (CONE - 1) + RING                  # frame H0 + 1 is the last poisoned one


@pytest.fixture(scope="module")
def live_waves():
    return noise((8, 256 * LIVE_HOPS), 89, 0.1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("v,limited", [(0, False), (5, True)])
def test_wave_stream_step(eng, win, live_waves, v, limited, kind):
    """N = 6 in calls of 1, 2 and 5 hops.  `limited`: atten_lim_db = 6 and level meters.  The live output is also the offline
    forward_wave of the same poisoned input one hop late, wherever the two are not both non-finite."""
    from gtcrn_micro_amd._lib import atten_lim_to_gain
    n, what = 6, f"wave_stream_step victim {v} limited={limited} {kind}"
    kw = dict(atten_lim_db=6.0, meters=True) if limited else {}
    x = live_waves[:n]
    xb = poisoned(x, (v, LIVE_SAMPLE), kind)

    def run(inp, k0=0, reset_at=None, meter_reset=True):
        st = eng.new_wave_state(inp.shape[0], win, **kw)
        before = {}
        if reset_at is not None:
            def cure():
                eng.wave_stream_reset(st, v, v + 1)
                if limited:
                    st.reset_meters(v, v + 1)
            before[reset_at] = cure
        if limited and meter_reset:
            before[METER_RESET] = lambda: st.reset_meters(v, v + 1)
        out = drive(lambda c: eng.wave_stream_step(st, c), inp, 256, calls_from(LIVE_CALLS, k0),
                    {k - k0: f for k, f in before.items()})
        return out.cpu().numpy(), snap(st, meters=limited)

    clean, cst = run(x)
    bad, bst = run(xb)
    check_blocks(clean, bad, v, LIVE_CONE, kind, what)
    same_states(bst, cst, slice(None), slice(None), f"{what}: P1 + P4 at the end")       # (meters included)
    off = eng.forward_wave(xb, win, dry_gain=atten_lim_to_gain(6.0) if limited else None).cpu().numpy()
    assert not bad[:, :256].any()
    assert IC.same_bits_or_both_nonfinite(bad[:, 256:], off[:, :256 * (LIVE_HOPS - 1)]), f"{what}: live != offline"
    k0 = H0 + 2
    cured, ust = run(xb, reset_at=k0, meter_reset=False)
    fresh, fst = run(xb[v:v + 1, 256 * k0:], k0=k0, meter_reset=False)             # (the victim alone, from hop k0 on)
    same(cured[v, 256 * k0:], fresh[0], f"{what}: P5 outputs after the reset")
    same_states(ust, fst, slice(v, v + 1), slice(0, 1), f"{what}: P5")
    same(cured[others(n, v)], clean[others(n, v)], f"{what}: P5 leaves the other rows alone")
    same_states(ust, cst, others(n, v), others(n, v), f"{what}: P5 leaves the other rows alone")


@pytest.mark.parametrize("kind", KINDS)
def test_wave_stream_step_slots(eng, win, live_waves, kind):
    """8 resident streams, 5 named per call (6, 1, 3, 0, 5), the victim slot 3 in the middle; slot 5 joins through
    wave_stream_reset_slots while the victim's cone passes.  Slots 2, 4 and 7 keep the bits of a state never stepped."""
    table, v, row, idle, join_at = [6, 1, 3, 0, 5], 3, 2, [2, 4, 7], H0 + 10
    tab = i32(table)
    what = f"wave_stream_step_slots {kind}"
    x = live_waves

    def run(inp, reset_at=None):
        st = eng.new_wave_state(8, win)
        eng.wave_stream_step(st, inp[:, -256:].contiguous())                 # every slot holds history
        start = snap(st)
        before = {join_at: lambda: eng.wave_stream_reset_slots(st, i32([5]))}
        if reset_at is not None:
            before[reset_at] = lambda: eng.wave_stream_reset_slots(st, i32([v, 5]), count=i32([1]))
        out = drive(lambda c: eng.wave_stream_step_slots(st, tab, c.contiguous()), inp[table], 256, [1] * LIVE_HOPS, before)
        return out.cpu().numpy(), snap(st), start

    xb = poisoned(x, (v, LIVE_SAMPLE), kind)
    clean, cst, start = run(x)
    bad, bst, _ = run(xb)
    check_blocks(clean, bad, row, LIVE_CONE, kind, what)
    same_states(bst, cst, slice(None), slice(None), f"{what}: P1 + P4 at the end")
    same_states(bst, start, idle, idle, f"{what}: P1 idle slots")
    k0 = H0 + 2
    cured, ust, _ = run(xb, reset_at=k0)
    st = eng.new_wave_state(1, win)
    fresh = drive(lambda c: eng.wave_stream_step(st, c), xb[v:v + 1, 256 * k0:], 256, [1] * (LIVE_HOPS - k0)).cpu().numpy()
    same(cured[row, 256 * k0:], fresh[0], f"{what}: P5 outputs after the reset")
    same_states(ust, snap(st), slice(v, v + 1), slice(0, 1), f"{what}: P5")
    same(cured[others(5, row)], clean[others(5, row)], f"{what}: P5 leaves the other rows alone")
    same_states(ust, cst, others(8, v), others(8, v), f"{what}: P5 leaves the other slots alone")


# ---- rate form: rate_stream_step ---------------------------------------------------------------------------------------------
# A sample of hop h at the caller's rate reaches, through the input filter (whose span and delay together stay below one hop),
# the 16 kHz hops h and h + 1; the wave step emits what those reach in its calls h .. h + 1 + CONE + 1; the output filter and
# its delay add less than one hop: the calls from h + CONE + 4 on are clean.  This is a worst-case count, not the exact edge:
# where the sample's filtered image stays inside hop h the output is clean about one hop earlier, and a value that lingered
# for that one hop longer than it should would pass here.
RATE_H0 = 1                          # inside the call of hops 1 .. 2; hop 3 starts a call
RATE_CLEAN = RATE_H0 + CONE + 4
assert LIVE_HOPS >= RATE_CLEAN + RING


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fs,highband", [(48000, None), (8000, None), (48000, 0.7)])
def test_rate_stream_step(eng, win, fs, highband, kind):
    """N = 3 streams at 48 and 8 kHz, 112 hops in calls of 1, 2 and 5, the victim in the middle; once with the high band, whose
    state is a delay line of the input and heals like the rest."""
    n, v, what = 3, 1, f"rate_stream_step fs={fs} highband={highband} {kind}"
    kw = dict(highband=highband) if highband is not None else {}
    hop = eng.new_rate_state(1, win, fs).hop
    x = noise((n, hop * LIVE_HOPS), fs // 10 + 3, 0.1)
    xb = poisoned(x, (v, hop * RATE_H0 + hop // 2 + 7), kind)

    def run(inp, k0=0, reset_at=None):
        st = eng.new_rate_state(inp.shape[0], win, fs, **kw)
        before = {reset_at - k0: lambda: eng.rate_stream_reset(st, v, v + 1)} if reset_at is not None else None
        out = drive(lambda c: eng.rate_stream_step(st, c), inp, hop, calls_from(LIVE_CALLS, k0), before)
        return out.cpu().numpy(), snap(st, hb=highband is not None)

    clean, cst = run(x)
    bad, bst = run(xb)
    assert ("hb" in cst) == (highband is not None) and "rate" in cst
    check_run_of_samples(clean, bad, v, hop * RATE_H0, hop * RATE_CLEAN, hop * (CONE - 1), kind, what)
    same_states(bst, cst, slice(None), slice(None), f"{what}: P1 + P4 at the end")
    k0 = 3
    cured, ust = run(xb, reset_at=k0)
    st = eng.new_rate_state(1, win, fs, **kw)
    fresh = drive(lambda c: eng.rate_stream_step(st, c), xb[v:v + 1, hop * k0:], hop, calls_from(LIVE_CALLS, k0)).cpu().numpy()
    same(cured[v, hop * k0:], fresh[0], f"{what}: P5 outputs after the reset")
    same_states(ust, snap(st, hb=highband is not None), slice(v, v + 1), slice(0, 1), f"{what}: P5")
    same(cured[others(n, v)], clean[others(n, v)], f"{what}: P5 leaves the other rows alone")
    same_states(ust, cst, others(n, v), others(n, v), f"{what}: P5 leaves the other rows alone")


# ---- packet forms ------------------------------------------------------------------------------------------------------------
# A packet form emits zeros(lead) ++ Y(x), lead < 512 samples at 16 kHz, Y the offline chain.  A sample of 16 kHz hop g makes Y
# non-finite up to block g + CONE at 16 kHz, one block more through the two filters: from 16 kHz sample 256 (g + CONE + 5) on
# the output is clean, and RING hops later the state is.  The count is a worst case with about one block of slack: at 16 kHz,
# where no filter runs, the exact edge is pinned separately by the identity with forward_wave and the cone of that offline
# run; at 48 and 44.1 kHz nothing pins it closer than this bound.
def packet_geometry(n16, poisoned_packet):
    g = (n16 * poisoned_packet + n16 // 2) // 256
    clean_from = -(-256 * (g + CONE + 5) // n16)                      # the first clean packet
    total = -(-256 * (g + CONE + 5 + RING) // n16)
    return clean_from, total


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fs,n", [(16000, 160), (48000, 480), (44100, 441)])
def test_packet_stream_step(eng, win, fs, n, kind):
    """A group of N = 3, the victim in the middle, the poison in packet 5; P5 resets the victim ahead of packet 8, where the
    group's phase is 0 again, so that a fresh one-stream group fed the packets from there on is the truth.  At 16 kHz the
    output is also zeros(lead) ++ forward_wave of the same poisoned input."""
    N, v, pk, k0 = 3, 1, 5, 8
    what = f"packet_stream_step fs={fs} packet={n} {kind}"
    n16 = n * 16000 // fs
    clean_from, K = packet_geometry(n16, pk)
    assert 256 * LIVE_HOPS >= n16 * K
    x = noise((N, n * K), fs // 10 + n, 0.1)
    xb = poisoned(x, (v, n * pk + n // 2 - 3), kind)
    assert 16000 * (n * pk + n // 2 - 3) // fs >= 257

    def run(inp, reset_at=None):
        st = eng.new_packet_state(N, win, n, fs)

        def cure():
            assert st.phase == 0
            eng.packet_stream_reset(st, v, v + 1)
        out = drive(lambda c: eng.packet_stream_step(st, c.contiguous()), inp, n, [1] * K,
                    {reset_at: cure} if reset_at is not None else None)
        return out.cpu().numpy(), snap(st)

    clean, cst = run(x)
    bad, bst = run(xb)
    assert cst["phase"].shape == (1,)
    check_run_of_samples(clean, bad, v, n * pk, n * clean_from, 256 * (CONE - 1) * fs // 16000, kind, what)
    same_states(bst, cst, slice(None), slice(None), f"{what}: P1 + P4 at the end")
    if fs == 16000:
        lead = 512 - gcd(n, 256)
        off = eng.forward_wave(xb, win).cpu().numpy()
        assert not bad[:, :lead].any()
        assert IC.same_bits_or_both_nonfinite(bad[:, lead:], off[:, :n * K - lead]), f"{what}: live != offline"
        if kind == "nan":
            g = (n * pk + n // 2 - 3) // 256
            got = IC.nonfinite_frames(off[v], block=256)
            assert got == {b: True for b in IC.cone_blocks(g, off.shape[1] // 256)}, (what, "P3", sorted(got))
    cured, ust = run(xb, reset_at=k0)
    st = eng.new_packet_state(1, win, n, fs)
    fresh = drive(lambda c: eng.packet_stream_step(st, c.contiguous()), xb[v:v + 1, n * k0:], n, [1] * (K - k0)).cpu().numpy()
    same(cured[v, n * k0:], fresh[0], f"{what}: P5 outputs after the reset")
    same_states(ust, snap(st), slice(v, v + 1), slice(0, 1), f"{what}: P5")
    same(cured[others(N, v)], clean[others(N, v)], f"{what}: P5 leaves the other rows alone")
    same_states(ust, cst, others(N, v), others(N, v), f"{what}: P5 leaves the other rows alone")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fs,n,highband", [(16000, 160, None), (48000, 480, 0.7)])
def test_packet_stream_step_slots(eng, win, fs, n, highband, kind):
    """6 resident slots at six different phases (slot s has taken s packets when the run starts), 4 named per call.  The victim,
    slot 2, is named in every call, in the middle of the table; its neighbour slot 3 loses every third packet; slots 0, 1, 4 and
    5 take turns.  P5 resets the victim through packet_stream_reset_slots ahead of its packet 8 of the run."""
    S, v, pk, k0 = 6, 2, 5, 8
    what = f"packet_stream_step_slots fs={fs} highband={highband} {kind}"
    kw = dict(highband=highband) if highband is not None else {}
    n16 = n * 16000 // fs
    clean_from, K = packet_geometry(n16, pk + v)                      # (the victim's packet pk of the run is its pk + v-th)
    clean_from -= v
    x = noise((S, n * (K + S)), fs // 10 + n + 1, 0.1)
    xb = poisoned(x, (v, n * (pk + v) + n // 2 - 3), kind)
    pool = [0, 1, 4, 5]

    def ids_of(t):
        a, b, c = pool[t % 4], pool[(t + 1) % 4], pool[(t + 2) % 4]
        return [a, v, 3 if t % 3 else c, b]

    def run(inp, reset_at=None):
        st = eng.new_packet_slot_state(S, win, n, fs, max_active=4, **kw)
        seen = [0] * S
        for s in range(S):                                            # slot s joins s packets before the run
            for _ in range(s):
                eng.packet_stream_step_slots(st, i32([s]), inp[s:s + 1, n * seen[s]:n * (seen[s] + 1)].contiguous())
                seen[s] += 1
        assert len(set(st.phase.tolist())) == S, st.phase.tolist()
        outs = [[] for _ in range(S)]
        for t in range(K):
            if reset_at == t:
                eng.packet_stream_reset_slots(st, i32([v, 3]), count=i32([1]))
            ids = ids_of(t)
            xin = torch.stack([inp[s, n * seen[s]:n * (seen[s] + 1)] for s in ids])
            out = eng.packet_stream_step_slots(st, i32(ids), xin)
            for i, s in enumerate(ids):
                outs[s].append(out[i].clone())
                seen[s] += 1
        return [torch.cat(o).cpu().numpy() for o in outs], snap(st, hb=highband is not None), seen

    clean, cst, seen = run(x)
    bad, bst, _ = run(xb)
    assert seen[v] == K + v and seen[3] < K + 3 - K // 4 and cst["phase"].shape == (S,)
    assert ("hb" in cst) == (highband is not None)
    for s in others(S, v):
        same(bad[s], clean[s], f"{what}: P1 slot {s}")
    check_run_of_samples(clean[v][None], bad[v][None], 0, n * pk, n * clean_from, 256 * (CONE - 1) * fs // 16000, kind, what)
    same_states(bst, cst, slice(None), slice(None), f"{what}: P1 + P4 at the end")
    cured, ust, _ = run(xb, reset_at=k0)
    st = eng.new_packet_state(1, win, n, fs, **kw)
    fresh = drive(lambda c: eng.packet_stream_step(st, c.contiguous()), xb[v:v + 1, n * (k0 + v):n * (K + v)], n,
                  [1] * (K - k0)).cpu().numpy()
    same(cured[v][n * k0:], fresh[0], f"{what}: P5 outputs after the reset")
    fst = snap(st, hb=highband is not None)
    assert int(ust["phase"][v]) == int(fst.pop("phase")[0]), f"{what}: P5 phase"
    phases = ust.pop("phase")
    same_states(ust, fst, slice(v, v + 1), slice(0, 1), f"{what}: P5")
    ust["phase"] = phases
    for s in others(S, v):
        same(cured[s], clean[s], f"{what}: P5 leaves slot {s} alone")
    same_states(ust, cst, others(S, v), others(S, v), f"{what}: P5 leaves the other slots alone")


# ---- Resampler (offline) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs_in,fs_out", [(48000, 16000), (16000, 48000), (44100, 16000)])
def test_resampler(eng, fs_in, fs_out):
    """Three rows of 6000 samples, row 1 holding 4000 and NaN behind them; a NaN at sample 3001 of row 0.  Row 0 is non-finite
    exactly where |j down - i0 up| <= half -- no tap is zero, so every output of the range reads the sample -- and keeps its
    bits elsewhere.  (scipy's own run is one sample wider at each end: it zero-pads the taps, and 0 * NaN is NaN.)"""
    from gtcrn_micro_amd._lib import resample_taps
    up, down, half, h64 = RC.design(fs_in, fs_out)
    u, d, h = resample_taps(fs_in, fs_out)
    assert (u, d, len(h)) == (up, down, 2 * half + 1) and (h != 0).all() and (h64 != 0).all()
    for pair in RC.PAIRS:                                             # the header states it for every supported pair
        assert (resample_taps(*pair)[2] != 0).all(), pair
    rs = eng.resampler(fs_in, fs_out)
    L, i0, lens = 6000, 3001, [6000, 4000, 6000]
    x = noise((3, L), fs_in // 100 + fs_out // 1000, 0.1)
    x[1, 4000:] = IC.QNAN
    n, n1 = rs.out_len(L), rs.out_len(4000)

    def run(inp):
        out = torch.full((3, n), -7.0, device="cuda")
        rs(inp, lengths=lens, out=out)
        return out.cpu().numpy()

    clean = run(x)
    bad = run(poisoned(x, (0, i0), "nan"))
    what = f"resample {fs_in}->{fs_out}"
    assert np.isfinite(clean[1, :n1]).all() and (clean[1, n1:] == -7.0).all(), what
    same(clean[1, :n1], rs(x[1, :4000].contiguous()), f"{what}: the short row alone")
    same(bad[1:], clean[1:], f"{what}: P1 rows 1 and 2")
    lo, hi = IC.resample_range(i0, up, down, half, n)
    assert 0 < lo < hi < n - 1
    same(bad[0, :lo], clean[0, :lo], f"{what}: before the range")
    same(bad[0, hi + 1:], clean[0, hi + 1:], f"{what}: behind the range")
    assert not np.isfinite(bad[0, lo:hi + 1]).any(), (what, int(np.isfinite(bad[0, lo:hi + 1]).sum()))
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[2]).all()
