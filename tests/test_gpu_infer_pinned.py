"""The fp32 inference path against the pinned float64 checker, stage by stage (oracle/infer_pinned.py).  Needs a real
MI355X: run with `-m gpu`.

Every stage tap of the HIP forward (k_front, k_encoder, k_gtcn_band x2, k_decoder<DBG>) is compared with the float64
eval graph's value computed FROM THE PREVIOUS HIP TAP, per clip and channel in that channel's own scale; the bound is
margin x what the float32 ATen port measures at the same stage, statistic and input.  One case per parameter set also
seeds every wrong layer of infer_pinned.BUGS into the checker and asserts that the real taps are rejected at that
stage and no other.  tests/test_infer_pinned_checker.py is the CPU stand-in of this file.  The stages that sit above
the default 1.5x / 2x, with the measured ratios and the cause of each, are listed at infer_pinned.MARGINS / ABS_FLOOR and
in DESIGN.md section 2.

The tap build keeps the time spans of an offline call (launch_decoder: a debug run is one SPANS launch, never split in
two; every share stores the taps of the frames it owns, the warm-up frames in front are left to their owner), so
(1, 90) and (5, 40) check taps written by shares that start inside an utterance."""
import numpy as np
import pytest

from conftest import load_params

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TAGS = ("dns3", "rand")
KINDS = ("white", "tilt")
# B = 2: one, two and three tiles per wave on either side of each switch (5/6, 10/11, 16/17) and two 16-frame chunks
# plus one frame; (1, 90) / (5, 40): workgroups in time spans
SHAPES = [(2, T) for T in (1, 2, 5, 6, 10, 11, 16, 17, 33)] + [(1, 90), (5, 40)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as graft
    graft.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def IP():
    from oracle import infer_pinned
    return infer_pinned


@pytest.fixture(scope="module")
def engines(dev):
    from gtcrn_micro_amd import Engine
    engs = {tag: Engine(load_params(tag), 0) for tag in TAGS}
    for e in engs.values():
        e.debug_enable(True)
    return engs


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hip_side(IP, eng, spec):
    B, _, T, _ = spec.shape
    out = eng.forward_spec(cu(spec)).cpu().numpy()
    return IP.engine_taps(eng, B, T), out


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tag", TAGS)
def test_every_stage_is_fp32_class_against_the_pinned_checker(IP, engines, tag, kind, B, T):
    spec = IP.make_input(kind, B, T, seed=100 * B + T)
    taps, out = hip_side(IP, engines[tag], spec)
    IP.assert_pinned_forward(load_params(tag), spec, taps, out, f"{tag} {kind} {B}x{T}", verbose=True)


@pytest.mark.parametrize("tag", TAGS)
def test_every_seeded_bug_is_rejected_on_the_hip_taps_at_its_own_stage_only(IP, engines, tag):
    """(2, 33): long enough for the history-edge slip of gtcn1.blocks.1 (frame 3) to exist."""
    blob = load_params(tag)
    spec = IP.make_input("white", 2, 33, seed=7)
    taps, out = hip_side(IP, engines[tag], spec)
    yard = IP.yardstick(blob, spec, taps)
    assert not IP.failing_stages(IP.measure(blob, spec, taps, out, yard=yard))
    got = {}
    for bug, (stage, what) in IP.BUGS.items():
        rows = IP.measure(blob, spec, taps, out, bug=bug, yard=yard)
        got[bug] = IP.failing_stages(rows)
        print(f"[{tag}] {bug}: rejected at {got[bug]}, {IP.distance(rows, stage):.3g}x the bound")
    assert got == {bug: [b.stage] for bug, b in IP.BUGS.items()}, got


@pytest.mark.parametrize("tag", TAGS)
def test_ring_form_output_and_last_chunk_stages(IP, engines, tag):
    """The (2, 33) input streamed through stream_step in chunks of 7, 16 and 10 frames (the ring form) with the taps on.
    A chunked call's taps hold its own frames only, so: the streamed OUTPUT of all 33 frames is judged at the checker's
    output stage (pinned to the offline taps, which the streamed path never wrote), and the last chunk's taps, spliced
    over frames 23..32 of the offline ones, are judged at every stage."""
    blob, eng = load_params(tag), engines[tag]
    spec = IP.make_input("white", 2, 33, seed=7)
    taps, _ = hip_side(IP, eng, spec)
    st = eng.new_state(2)
    dspec, outs, t = cu(spec), [], 0
    for n in (7, 16, 10):
        outs.append(eng.stream_step(st, dspec[:, :, t:t + n]))
        t += n
    out = torch.cat(outs, 2).cpu().numpy()
    last = IP.engine_taps(eng, 2, 10)
    rows = [r for r in IP.measure(blob, spec, taps, out) if r.stage == "out"]
    show_rows = [IP.fmt(r) for r in rows]
    print(f"[{tag} ring] " + "; ".join(show_rows))
    assert all(r.ok for r in rows), show_rows
    spliced = {n: np.concatenate([taps[n][:, :, :23], last[n]], axis=2) for n in IP.ENGINE_TAPS}
    IP.assert_pinned_forward(blob, spec, spliced, out, f"{tag} ring, last chunk", verbose=True)
