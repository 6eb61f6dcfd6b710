"""The int8-weight / fp16-activation variant, stage by stage: the fp16 records the kernels hand over (en0..en4, gtcn1,
sum4 = gtcn2(x) + en4) and the decoder's stage taps (de0..de4, k_decoder<DBG, ., ., Q>) against QuantPort("f64") pinned
to the device's own taps (tests/quant_cases.py: accept_stages) -- and, without any tolerance, what the taps are: the
tapped build computes the plain build's bits, every tap holds fp16 numbers, a clip's taps do not depend on its batch, the
taps follow the variant of the last forward, and the two refusals."""
import numpy as np
import pytest

import quant_cases as QC
from conftest import load_params

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TAGS = ("dns3", "rand")
HANDOFFS = ("en0", "en1", "en2", "en3", "en4", "gtcn1", "sum4")
DECODER = ("de0", "de1", "de2", "de3", "de4")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as graft
    graft.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engines(dev):
    from gtcrn_micro_amd import Engine
    return {tag: Engine(load_params(tag), 0) for tag in TAGS}


def _scales():
    from oracle.quant_port import CALIB_SCALE
    return CALIB_SCALE, CALIB_SCALE * 2 ** 0.5


def _noise(seed, B, T, amp=0.3):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal((B, 257, T, 2)) * amp).astype(np.float32)).cuda()


def _is_fp16(a):
    return np.array_equal(a, a.astype(np.float16).astype(np.float32))


# ---- a. every stage under the pinned acceptance function ------------------------------------------------------------
@pytest.mark.parametrize("case", [c for tag in TAGS for c in QC.stage_cases(tag)], ids=repr)
def test_every_stage_against_the_pinned_checker(engines, case):
    for seed in case.seeds:
        taps = QC.device_taps(engines[case.tag], case, seed)
        ok, rep = QC.accept_stages(taps, case, seed)
        for st, (a, s, r, fl) in rep.items():
            print(f"{case.name} seed {seed} {st:5s} kernel / floor  L2 {r[0]:.2f}  frame {r[1]:.2f}  frac {r[2]:.2f}   "
                  f"(statistics {s[0]:.2e} {s[1]:.2e} {s[2]:.2e}, floors {fl[0]:.2e} {fl[1]:.2e} {fl[2]:.2e})")
        assert ok, (case, seed, QC.K_STAGE, QC.stage_failures(rep))


# ---- b. the stage-tap instantiation vs the plain one ----------------------------------------------------------------
@pytest.mark.parametrize("scales", [(0.0, 0.0), _scales()], ids=["fp16", "int8"])
@pytest.mark.parametrize("T", [3, 8, 17, 40])
def test_debug_tap_build_output_equals_plain_instantiation(dev, T, scales):
    """The stage evidence above comes from k_decoder<DBG = true, ., ., Q = true>, a differently scheduled binary than
    the k_decoder<false, ., ., true> every other caller runs: their OUTPUTS must be the same bits."""
    from gtcrn_micro_amd import Engine
    p = load_params("rand")
    plain, tapped = Engine(p, 0), Engine(p, 0)
    tapped.debug_enable(True)
    spec = _noise(T, 3, T, 0.4)
    a, b = plain.forward_spec_quant(spec, *scales), tapped.forward_spec_quant(spec, *scales)
    assert torch.equal(a, b), float((a - b).abs().max())
    assert tapped.tap("de4", 2, T).shape == (2, T, 129)


# ---- c. what the taps are -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_every_tap_holds_fp16_numbers_and_en_taps_ignore_the_batch(engines, tag):
    eng = engines[tag]
    case = QC.BY_NAME[f"{tag}-B3-T17"]
    taps = QC.device_taps(eng, case, 0)
    for st, a in taps.items():
        assert np.isfinite(a).all() and _is_fp16(a), st
        assert float(np.abs(a).max()) > 0, st
    x = case.input(0)
    for b in range(3):
        eng.debug_enable(True)
        eng.forward_spec_quant(torch.from_numpy(x[b:b + 1]).cuda())
        for st in HANDOFFS + DECODER:
            assert np.array_equal(eng.tap(st, 0, 17), taps[st][b]), (st, b)
        eng.debug_enable(False)


def test_taps_follow_the_variant_of_the_last_forward(dev):
    """fp32 taps after a quant forward read fp32 again, and the reverse; sum4 of an fp32 forward is the stored sum the
    gtcn2 tap subtracts en4 from."""
    from gtcrn_micro_amd import Engine
    p = load_params("rand")
    mixed, only32, onlyq = Engine(p, 0), Engine(p, 0), Engine(p, 0)
    for e in (mixed, only32, onlyq):
        e.debug_enable(True)
    x, T = _noise(5, 2, 17), 17
    names32 = HANDOFFS[:-1] + ("gtcn2",) + DECODER
    only32.forward_spec(x)
    onlyq.forward_spec_quant(x)
    want32 = {st: only32.tap(st, 1, T) for st in names32 + ("sum4",)}
    wantq = {st: onlyq.tap(st, 1, T) for st in HANDOFFS + DECODER}
    assert not _is_fp16(want32["en1"]) and not _is_fp16(want32["de1"])
    assert np.array_equal(want32["gtcn2"], want32["sum4"] - want32["en4"])
    mixed.forward_spec_quant(x)
    assert np.array_equal(mixed.tap("en2", 1, T), wantq["en2"])
    mixed.forward_spec(x)
    for st in names32:
        assert np.array_equal(mixed.tap(st, 1, T), want32[st]), st
    mixed.forward_spec_quant(x)
    for st in HANDOFFS + DECODER:
        assert np.array_equal(mixed.tap(st, 1, T), wantq[st]), st


def test_tap_argument_errors(dev):
    from gtcrn_micro_amd import Engine
    from gtcrn_micro_amd._lib import GtcrnError
    eng = Engine(load_params("rand"), 0)
    x = _noise(6, 1, 5)
    eng.forward_spec_quant(x)
    for st in HANDOFFS + DECODER:                                     # a quant forward without the taps enabled: none
        with pytest.raises(GtcrnError, match="gtcrn_debug_enable"):
            eng.tap(st, 0, 5)
    eng.debug_enable(True)
    for st in HANDOFFS + DECODER:                                     # enabling them AFTER the forward does not help
        with pytest.raises(GtcrnError, match="gtcrn_debug_enable"):
            eng.tap(st, 0, 5)
    eng.forward_spec_quant(x)
    assert eng.tap("sum4", 0, 5).shape == (16, 5, 33) and eng.tap("de0", 0, 5).shape == (16, 5, 33)
    with pytest.raises(GtcrnError, match="sum4"):                     # gtcn2(x) + en4 is rounded: no un-adding
        eng.tap("gtcn2", 0, 5)
    with pytest.raises(GtcrnError, match="unknown tap name"):
        eng.tap("sum3", 0, 5)
    with pytest.raises(GtcrnError):
        eng.tap("en0", 1, 5)                                          # batch index out of range
    eng.debug_enable(False)
    for st in DECODER:                                                # the decoder taps need it at the time of the tap too
        with pytest.raises(GtcrnError, match="gtcrn_debug_enable"):
            eng.tap(st, 0, 5)
    assert eng.tap("en0", 0, 5).shape == (16, 5, 65)
