"""Edges of the int8-weight / fp16-activation variant (gtcrn_forward_spec_quant / gtcrn_forward_wave_quant), black box:
lengths round the 16-frame chunk under the flip-noise acceptance function of tests/quant_cases.py, and -- without any
tolerance -- prefix invariance, causality, batch position, strided views and the two int8 boundary quantisers."""
import ctypes

import numpy as np
import pytest

import quant_cases as QC
from conftest import load_params

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TAGS = ("dns3", "rand")
SENTINEL = -7.25


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


def _host_quant(x, scale):
    """The contract's quantiser on the host, in float32: clip(rint(x / step), -128, 127) * step, ties to even."""
    from oracle.quant_port import quant_step
    step = quant_step(scale)
    x = np.asarray(x, np.float32)
    return (np.clip(np.rint(x / step), np.float32(-128), np.float32(127)) * step).astype(np.float32)


def _noise(seed, B, T, amp=0.3):
    return (np.random.default_rng(seed).standard_normal((B, 257, T, 2)) * amp).astype(np.float32)


# ---- a. lengths round the chunk, under the acceptance function ------------------------------------------------------
@pytest.mark.parametrize("case", QC.CASES, ids=repr)
def test_lengths_round_the_chunk(engines, case):
    """T = 1 .. 49 x B = 1, 3 at amplitude 0.3, T = 49 at 1.5, and the two boundary inputs (loud with the int8
    boundary, exact quantiser ties): forward_spec_quant against QuantPort(acc="f64"), every seed of the case."""
    pairs, floors = QC.reference(case)
    eng = engines[case.tag]
    for x, ref, _ in pairs:
        got = eng.forward_spec_quant(torch.from_numpy(x).cuda(), case.in_scale, case.out_scale).cpu().numpy()
        ok, s, ratios = QC.accept(got, ref, floors)
        print(f"{case.name}: kernel / floor  L2 {ratios[0]:.2f}  frame {ratios[1]:.2f}  frac {ratios[2]:.2f}   "
              f"(floors {floors[0]:.2e} {floors[1]:.2e} {floors[2]:.2e})")
        assert ok, (case, s, floors, ratios, QC.K)
        if case.out_scale == 0:
            assert np.array_equal(got, got.astype(np.float16).astype(np.float32))       # every value an fp16 number


# ---- b. prefix invariance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", [(0.0, 0.0), _scales()], ids=["fp16", "int8"])
@pytest.mark.parametrize("tag", TAGS)
def test_prefix_invariance(engines, tag, scales):
    """Causal with zero initial history: the first T' frames of the T = 49 result are the result of the first T' frames
    alone, bit for bit -- wherever the last chunk ends."""
    eng = engines[tag]
    x = torch.from_numpy(_noise(21, 3, 49)).cuda()
    full = eng.forward_spec_quant(x, *scales)
    for T in QC.LENGTHS:
        part = eng.forward_spec_quant(x[:, :, :T].contiguous(), *scales)
        assert torch.equal(part, full[:, :, :T]), (tag, T)


# ---- c. causality ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_causality(engines, tag):
    eng = engines[tag]
    x = torch.from_numpy(_noise(22, 2, 40)).cuda()
    y = eng.forward_spec_quant(x)
    for t0 in (15, 16, 17, 32):
        x2 = x.clone()
        x2[:, :, t0] = torch.from_numpy(_noise(23 + t0, 2, 1))[:, :, 0].cuda()
        y2 = eng.forward_spec_quant(x2)
        assert torch.equal(y2[:, :, :t0], y[:, :, :t0]), (tag, t0)
        assert not torch.equal(y2[:, :, t0:], y[:, :, t0:]), (tag, t0)


# ---- d. batch position ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", [(0.0, 0.0), _scales()], ids=["fp16", "int8"])
@pytest.mark.parametrize("tag", TAGS)
def test_batch_position(engines, tag, scales):
    eng = engines[tag]
    x = torch.from_numpy(_noise(24, 3, 17)).cuda()
    x[1] = 0.0
    x[2] *= 3.0
    y = eng.forward_spec_quant(x, *scales)
    for b in range(3):
        assert torch.equal(y[b:b + 1], eng.forward_spec_quant(x[b:b + 1].contiguous(), *scales)), (tag, b)
    assert float(y[1].abs().max()) < 1e-4


# ---- e. strided views -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", [(0.0, 0.0), _scales()], ids=["fp16", "int8"])
@pytest.mark.parametrize("tag", TAGS)
def test_strided_views(engines, tag, scales):
    eng = engines[tag]
    B, T = 2, 17
    x = torch.from_numpy(_noise(25, B, T)).cuda()
    want = eng.forward_spec_quant(x, *scales)
    x_fm = x.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)           # stored (B,T,257,2)
    assert not x_fm.is_contiguous()
    assert torch.equal(eng.forward_spec_quant(x_fm, *scales), want)
    # frame-major output inside a larger sentinel-filled buffer: two spare frames in front of every utterance, three behind
    big = torch.full((B, T + 5, 257, 2), SENTINEL, device="cuda")
    view = big[:, 2:2 + T].permute(0, 2, 1, 3)
    ret = eng.forward_spec_quant(x_fm, *scales, out=view)
    assert ret.data_ptr() == view.data_ptr()
    assert torch.equal(view, want)
    assert bool((big[:, :2] == SENTINEL).all()) and bool((big[:, 2 + T:] == SENTINEL).all())
    # bin-major output with spare frames at the end of every bin row
    big = torch.full((B, 257, T + 3, 2), SENTINEL, device="cuda")
    eng.forward_spec_quant(x, *scales, out=big[:, :, :T])
    assert torch.equal(big[:, :, :T], want) and bool((big[:, :, T:] == SENTINEL).all())


# ---- f. input quantiser, exactly ------------------------------------------------------------------------------------
def _quantiser_probe(s_in):
    """(1,257,17,2) input: noise that saturates at both ends, exact ties (k + 0.5) * step for even and odd k, the
    neighbours of +-128 * step, +127 * step and of the clipping ties, zeros and denormals."""
    from oracle.quant_port import quant_step
    step = quant_step(s_in)
    x = _noise(26, 1, 17, 4.0)
    flat = x.reshape(-1)
    k = np.arange(-131, 131, dtype=np.float32)
    ties = ((k + np.float32(0.5)) * step).astype(np.float32)
    exact = (ties / step) == (k + np.float32(0.5))                  # ties of the float32 quotient the contract forms
    ties, k = ties[exact], k[exact]
    assert np.any(k % 2 == 0) and np.any(k % 2 == 1) and ties.size > 100
    edges = []
    for v in (-128.5, -128.0, -127.5, -127.0, 126.5, 127.0, 127.5, 128.0):
        e = np.float32(np.float32(v) * step)
        edges += [e, np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf))]
    small = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, 6e-8, -6e-8, 6.1e-5, np.float32(step) / 2]
    special = np.concatenate([ties, -ties, np.array(edges, np.float32), np.array(small, np.float32)])
    pos = np.random.default_rng(27).permutation(flat.size)[:special.size * 3]
    flat[pos] = np.tile(special, 3)                                 # at three places each, all over bins and frames
    return x


@pytest.mark.parametrize("with_out", [False, True], ids=["fp16-out", "int8-out"])
@pytest.mark.parametrize("tag", TAGS)
def test_input_quantiser_exact(engines, tag, with_out):
    from oracle.quant_port import quant_step
    eng = engines[tag]
    s_in, s_out = _scales()
    s_out = s_out if with_out else 0.0
    x = _quantiser_probe(s_in)
    qx = _host_quant(x, s_in)
    assert 0 < np.mean(np.abs(qx) >= np.float32(127) * quant_step(s_in)) < 0.5         # some saturate, most do not
    got = eng.forward_spec_quant(torch.from_numpy(x).cuda(), s_in, s_out)
    want = eng.forward_spec_quant(torch.from_numpy(qx).cuda(), 0.0, s_out)
    assert torch.equal(got, want), (tag, int((got != want).sum()))


# ---- g. output quantiser, exactly -----------------------------------------------------------------------------------
# the trained model takes some 25 dB off noise, the random one nothing: an output scale per parameter set, such that
# between a few per cent and a third of the values clip at amplitude 12 (worked out with the CPU checker)
OUT_SCALE_DIV = {"dns3": 16.0, "rand": 1.0}


@pytest.mark.parametrize("s_in_on", [False, True], ids=["fp16-in", "int8-in"])
@pytest.mark.parametrize("tag", TAGS)
def test_output_quantiser_exact(engines, tag, s_in_on):
    from oracle.quant_port import quant_step
    eng = engines[tag]
    s_in, s_out = _scales()
    s_in, s_out = (s_in if s_in_on else 0.0), s_out / OUT_SCALE_DIV[tag]
    x = torch.from_numpy(_noise(28, 2, 17, 12.0)).cuda()
    got = eng.forward_spec_quant(x, s_in, s_out).cpu().numpy()
    plain = eng.forward_spec_quant(x, s_in, 0.0).cpu().numpy()
    want = _host_quant(plain, s_out)
    step = quant_step(s_out)
    sat = float(np.mean((want == np.float32(127) * step) | (want == np.float32(-128) * step)))
    print(f"{tag}: saturating fraction {sat:.3f}")
    assert 0.0 < sat < 0.5
    assert np.array_equal(got, want), (tag, int((got != want).sum()))
    assert np.array_equal(np.signbit(got), np.signbit(want))


# ---- h. wave path at small size -------------------------------------------------------------------------------------
@pytest.mark.parametrize("hops", [1, 16, 17])
@pytest.mark.parametrize("tag", TAGS)
def test_wave_path_small(engines, tag, hops):
    """forward_wave_quant on B = 2 clips of 256 * hops samples against oracle STFT -> QuantPort(acc="f64") -> oracle
    iSTFT, e(t) per hop.  The shortest clip the STFT admits is 257 samples (reflect padding, GTCRN_ERR_ARG below): at
    hops = 1 the 256-sample clip has to be refused and the check runs on 257 samples (two frames, one hop out)."""
    from gtcrn_micro_amd import GtcrnError
    from oracle import oracle as O
    eng = engines[tag]
    win = torch.from_numpy(O.window(0)).cuda()
    L = 256 * hops
    if hops == 1:
        with pytest.raises(GtcrnError):
            eng.forward_wave_quant(torch.zeros(2, L, device="cuda"), win)
        L = 257
    # seeds as in the spectrogram cases: eight where the utterance is a frame or two (a single draw is anywhere between
    # no flip at all and the tail of the avalanche), two otherwise
    waves = [(np.random.default_rng(30 + s).standard_normal((2, L)) * 0.1).astype(np.float32)
             for s in range(8 if hops == 1 else 2)]
    specs = [O.stft(w, O.window(0)) for w in waves]
    refs = [O.istft(QC.port(tag, "f64").forward(s), O.window(0)).reshape(2, hops, 256) for s in specs]
    f32 = [O.istft(QC.port(tag, "f32").forward(s), O.window(0)).reshape(2, hops, 256) for s in specs]
    floors = tuple(max(v) for v in zip(*(QC.stats(a, r, frame_axes=(2,)) for a, r in zip(f32, refs))))
    for w, ref in zip(waves, refs):
        wt = torch.from_numpy(w).cuda()
        y = eng.forward_wave_quant(wt, win)
        assert y.shape == (2, 256 * hops)
        ok, s, ratios = QC.accept(y.cpu().numpy().reshape(2, hops, 256), ref, floors, frame_axes=(2,))
        print(f"wave {tag} hops={hops}: kernel / floor  L2 {ratios[0]:.2f}  hop {ratios[1]:.2f}  frac {ratios[2]:.2f}   "
              f"(floors {floors[0]:.2e} {floors[1]:.2e} {floors[2]:.2e})")
        assert ok, (tag, hops, s, floors, ratios, QC.K)
        for b in range(2):
            assert torch.equal(y[b], eng.forward_wave_quant(wt[b].contiguous(), win)), (tag, hops, b)


# ---- i. argument errors ---------------------------------------------------------------------------------------------
def _header_enum(name):
    """The value the public header gives an error code."""
    import pathlib
    import re
    text = (pathlib.Path(__file__).resolve().parent.parent / "include" / "gtcrn_micro_hip.h").read_text()
    return int(re.search(rf"\b{name}\s*=\s*(-?\d+)", text).group(1))


def test_argument_errors(engines):
    from gtcrn_micro_amd import _lib
    L = _lib.lib()
    eng = engines["dns3"]
    B, T = 2, 5
    x = torch.from_numpy(_noise(29, B, T)).cuda()
    out = torch.full((B, 257, T, 2), SENTINEL, device="cuda")
    sb, sf, st = x.stride(0), x.stride(1), x.stride(2)
    ERR_ARG, ERR_STATE = _header_enum("GTCRN_ERR_ARG"), _header_enum("GTCRN_ERR_STATE")
    assert ERR_ARG < 0 and ERR_STATE < 0 and ERR_ARG != ERR_STATE

    def call(outp=None, T_=T, si=0.0, so=0.0):
        return L.gtcrn_forward_spec_quant(eng._h, x.data_ptr(), sb, sf, st, out.data_ptr() if outp is None else outp,
                                          sb, sf, st, B, T_, si, so, None)
    assert call(si=-1.0) == ERR_ARG and call(so=-1e-3) == ERR_ARG and call(si=-1.0, so=-1.0) == ERR_ARG
    assert call(T_=0) == ERR_ARG and call(T_=-3) == ERR_ARG
    assert call(outp=ctypes.c_void_p(None)) == ERR_ARG
    wave = torch.zeros(2, 1024, device="cuda")
    wout = torch.full((2, 1024), SENTINEL, device="cuda")
    win = torch.hann_window(512, device="cuda").pow(0.5)
    for si, so in ((-1.0, 0.0), (0.0, -1.0)):
        assert L.gtcrn_forward_wave_quant(eng._h, wave.data_ptr(), wout.data_ptr(), 2, 1024, win.data_ptr(), si, so,
                                          None) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((wout == SENTINEL).all())
    # the stage taps read fp32 hand-offs: after a quant forward they refuse
    eng.forward_spec_quant(x)
    dst = np.empty(16 * T * 65, np.float32)
    assert L.gtcrn_debug_tap(eng._h, b"en0", 0, dst.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), dst.size) == ERR_STATE
