"""The pinned float64 checker of the fp32 inference path (oracle/infer_pinned.py), on the CPU.

The float32 port's own unpinned stage tensors stand in for the HIP taps (what tests/test_pinned_checker.py does for
training): every stage must pass, every seeded wrong layer (infer_pinned.BUGS) must be rejected at its own stage and at
no other, the table that maps the engine's tap names onto the port's must be complete, and the per-channel figure must
see an error in a quiet channel that the stage metric of test_forward_every_stage_vs_golden (max|a-b| / max|b| against
REG_STAGE) does not.  tests/test_gpu_infer_pinned.py applies the same functions to the real taps."""
import os
import re

import numpy as np
import pytest

from conftest import REG_STAGE, ROOT, load_params, rel_err

torch = pytest.importorskip("torch")

CASES = [(tag, kind, B, T) for tag in ("dns3", "rand") for kind, B, T in
         (("white", 2, 17), ("tilt", 2, 16), ("white", 1, 1), ("tilt", 2, 6))]


@pytest.fixture(scope="module")
def IP():
    from oracle import infer_pinned
    return infer_pinned


@pytest.fixture(scope="module")
def stand_ins(IP):
    """{case: (blob, spec, taps, out)} -- computed once, never modified."""
    res = {}
    for tag, kind, B, T in CASES:
        blob = load_params(tag)
        spec = IP.make_input(kind, B, T, seed=T)
        res[tag, kind, B, T] = (blob, spec) + IP.stand_in(blob, spec)
    return res


def test_name_table_is_complete(IP, stand_ins):
    """Every tap the engine serves has a port name, the port records it, and what the port records beyond the table is
    exactly the interior the engine does not hand out."""
    src = open(os.path.join(ROOT, "gtcrn_micro_amd", "csrc", "api.cpp")).read()
    served = set(re.findall(r'nm == "(\w+)"', src[src.index("long gtcrn_debug_tap("):src.index("long gtcrn_debug_stamps(")]))
    assert served == set(IP.ENGINE_TAPS), served ^ set(IP.ENGINE_TAPS)
    assert IP.ENGINE_TO_PORT["sum4"] == "sum0" and all(k == v for k, v in IP.ENGINE_TO_PORT.items() if k != "sum4")
    blob, spec, taps, out = stand_ins["dns3", "white", 2, 17]
    own = IP.pinned_run(blob, spec, taps)
    assert sorted(own) == sorted(list(IP.ENGINE_TO_PORT.values()) + list(IP.PORT_INTERIOR) + ["out"])
    assert set(IP.STAGES) == (set(IP.ENGINE_TAPS) - {"sum4"}) | {"out"}
    assert {b.stage for b in IP.BUGS.values()} <= set(IP.STAGES)
    for n in IP.ENGINE_TAPS:
        assert taps[n].shape == own[IP.ENGINE_TO_PORT[n]].shape, n
    assert all(m[0] >= IP.DEFAULT_MARGIN[0] and m[1] >= IP.DEFAULT_MARGIN[1] for m in IP.MARGINS.values())
    assert set(IP.MARGINS) | set(IP.ABS_FLOOR) <= set(IP.STAGES)


@pytest.mark.parametrize("tag,kind,B,T", CASES)
def test_every_stage_passes_on_the_float32_stand_in(IP, stand_ins, tag, kind, B, T):
    blob, spec, taps, out = stand_ins[tag, kind, B, T]
    rows = IP.assert_pinned_forward(blob, spec, taps, out, f"{tag} {kind} {B}x{T}")
    assert {r.stage for r in rows} == set(IP.STAGES)
    # the pin is what makes a stage's figure its own: pinned, the stand-in IS the float32 port stage by stage
    assert all(r.worst == r.port for r in rows), [IP.fmt(r) for r in rows if r.worst != r.port]
    assert max(r.hip for r in rows if r.stat == "rms") < 1e-5       # fp32-class at all (measured <= 2e-6)


@pytest.mark.parametrize("tag", ["dns3", "rand"])
def test_correctly_rounded_stages_pass(IP, stand_ins, tag):
    """A HIP side that could not be better -- every stage the float64 graph's own value rounded to fp32 once -- passes:
    the yardstick is never tighter than one rounding."""
    blob, spec, _, _ = stand_ins[tag, "white", 2, 17]
    taps, out = IP.stand_in(blob, spec, dtype=torch.float64)
    taps["sum4"] = taps["gtcn2"] + taps["en4"]                      # as a kernel stores it: the fp32 sum of its fp32 taps
    IP.assert_pinned_forward(blob, spec, taps, out, tag)


def test_the_kernels_rounded_slope_is_allowed_for_and_twice_it_is_not(IP, stand_ins):
    """The kernels' PReLU slope is fl32(a - 1) + 1 (kernels.hip prelu4).  A HIP side that is the float64 graph ON THOSE
    SLOPES, every stage rounded to fp32 once, is far over the port in dns3's quiet en0 and de3 channels (slopes 0.0131
    and 0.00122: the slope's relative error is 2e-6 and 1e-5) and passes, through the slope allowance alone; with twice
    the kernels' slope error it fails, at those two stages."""
    blob, spec, _, _ = stand_ins["dns3", "white", 2, 17]
    for mult, want in ((1.0, []), (2.0, ["en0", "de3"])):
        taps, out = IP.stand_in(blob, spec, dtype=torch.float64, slope_error=mult)
        taps["sum4"] = taps["gtcn2"] + taps["en4"]
        rows = IP.measure(blob, spec, taps, out)
        raw = IP.ratios(rows)
        print(f"slope error x{mult}: en0 {raw['en0'][0][0]:.2f}, de3 {raw['de3'][0][0]:.2f} x the port's rms figure")
        assert raw["en0"][0][0] > 3 and raw["de3"][0][0] > 5          # (measured 7 and 10 at x1)
        assert IP.failing_stages(rows) == want, [IP.fmt(r) for r in rows if not r.ok]


def test_a_seeded_bug_never_writes_through_to_the_blob(IP, stand_ins):
    blob, spec, taps, out = stand_ins["rand", "white", 1, 1]
    keep = blob.copy()
    for bug in IP.BUGS:
        for dtype in (torch.float32, torch.float64):
            IP._Checker(blob, dtype, None, bug)
    assert np.array_equal(keep.view(np.uint32), blob.view(np.uint32))


@pytest.mark.parametrize("tag,kind,B,T", [c for c in CASES if c[3] >= 16])
def test_every_seeded_bug_is_rejected_at_its_own_stage_only(IP, stand_ins, tag, kind, B, T):
    blob, spec, taps, out = stand_ins[tag, kind, B, T]
    yard = IP.yardstick(blob, spec, taps)
    assert not IP.failing_stages(IP.measure(blob, spec, taps, out, yard=yard))
    for bug, (stage, what) in IP.BUGS.items():
        rows = IP.measure(blob, spec, taps, out, bug=bug, yard=yard)
        print(f"{tag} {kind}: {bug} rejected at {IP.failing_stages(rows)}, {IP.distance(rows, stage):.3g}x the bound")
        assert IP.failing_stages(rows) == [stage], (bug, what, IP.failing_stages(rows))


def test_sum4_mismatch_is_reported(IP, stand_ins):
    blob, spec, taps, out = stand_ins["dns3", "white", 2, 17]
    bad = dict(taps)
    bad["sum4"] = taps["sum4"].copy()
    bad["sum4"][1, 3, 2, 7] = np.nextafter(bad["sum4"][1, 3, 2, 7], np.float32(np.inf))
    with pytest.raises(AssertionError, match=r"sum4 != fp32\(gtcn2 \+ en4\) at 1 of .* \(1, 3, 2, 7\)"):
        IP.assert_pinned_forward(blob, spec, bad, out)


def test_per_channel_figure_sees_a_quiet_channel_the_max_norm_does_not(IP, stand_ins):
    """de3 of the dns3 weights on white noise: the loudest channel is > 100x the quietest.  An error of 1e-3 of the quiet
    channel's rms in that channel alone is ~1e-6 of the stage's maximum -- below REG_STAGE, the whole-tensor max-norm of
    test_forward_every_stage_vs_golden passes it -- and fails the pinned check at de3, naming the channel."""
    blob, spec, taps, out = stand_ins["dns3", "white", 2, 17]
    rms = np.sqrt((taps["de3"].astype(np.float64) ** 2).mean(axis=(0, 2, 3)))
    quiet = int(np.argmin(rms))
    assert rms.max() > 100 * rms[quiet]
    bad = dict(taps)
    bad["de3"] = taps["de3"].copy()
    sign = np.where(np.arange(65) % 2 == 0, 1.0, -1.0).astype(np.float32)
    bad["de3"][:, quiet] += np.float32(1e-3 * rms[quiet]) * sign
    assert rel_err(bad["de3"], taps["de3"]) < REG_STAGE
    rows = IP.measure(blob, spec, bad, out)
    assert "de3" in IP.failing_stages(rows)
    worst = [r for r in rows if r.stage == "de3" and r.stat == "rms"][0]
    assert worst.group == quiet and 0.5e-3 < worst.hip < 2e-3 and worst.hip > 10 * worst.bound
    with pytest.raises(AssertionError, match=f"de3: clip . channel {quiet}: rms error"):
        IP.assert_pinned_forward(blob, spec, bad, out)
