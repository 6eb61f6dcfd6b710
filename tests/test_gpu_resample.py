"""gtcrn_resample on the GPU against the float64 checker (tests/resample_checker.py: scipy.signal.resample_poly with the
library's own taps), every supported pair of rates; the int16 forms; batches of unequal lengths; and
Engine.forward_wave_rate (contract: include/gtcrn_micro_hip.h)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, TOL, load_params, rel_err
import resample_checker as RC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 7.0


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
def examples():
    return np.load(os.path.join(GOLDEN, "examples_full.npz"))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_rows(rs, taps, x, lengths, what):
    """x (B,L) float32 numpy, lengths per row: the batched call against the checker row by row, within the fp32
    dot-product bound (n + 1) 2^-24 sum |x_i| |h_k| (plus 2^-50 of the same sum for the float64 reference's own rounding);
    untouched beyond each row's output length; each row equal to itself resampled alone, bit for bit."""
    up, down, h = taps
    B, L = x.shape
    nmax = RC.out_len(L, up, down)
    out = torch.full((B, nmax + 5), SENTINEL, device="cuda")
    rs(cu(x), lengths=None if lengths is None else list(lengths), out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    worst = 0.0
    for b in range(B):
        lb = L if lengths is None else int(lengths[b])
        n = RC.out_len(lb, up, down)
        assert (got[b, n:] == SENTINEL).all(), (what, b, "wrote beyond the row's output length")
        if lb == 0:
            continue
        want = RC.resample64(x[b, :lb], up, down, h)
        assert want.size == n
        s = RC.dot_bound(x[b, :lb], up, down, h)
        bound = s * (1 + 2.0 ** -26)
        err = np.abs(got[b, :n].astype(np.float64) - want)
        assert (err <= bound).all(), (what, b, float((err - bound).max()))
        nz = bound > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz]).max()))
        alone = rs(cu(x[b, :lb]))
        assert alone.shape == (n,)
        assert torch.equal(alone, out[b, :n]), (what, b, "row in a batch != the row alone")
    print(f"{what}: worst error / bound = {worst:.3f}")
    return got


@pytest.mark.parametrize("fs_in,fs_out", RC.PAIRS)
def test_resample_matches_the_float64_checker(dev, fs_in, fs_out):
    """Noise, a 1 kHz sine and a batch of unequal lengths -- shorter than the filter, length 1, L * up not divisible by
    down, several tiles of outputs -- B = 1 and B = 8."""
    from gtcrn_micro_amd._lib import Resampler, resample_taps
    taps = resample_taps(fs_in, fs_out)
    up, down, _ = taps
    rs = Resampler(fs_in, fs_out, 0)
    rng = np.random.default_rng(fs_in + 3 * fs_out)
    L = 12007
    assert (L * up) % down or down == 1, "the length must leave a partial last output period"
    noise = (rng.standard_normal((1, L)) * 0.3).astype(np.float32)
    check_rows(rs, taps, noise, None, f"{fs_in}->{fs_out} noise B=1")
    t = np.arange(L) / fs_in
    sine = (0.5 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)[None]
    got = check_rows(rs, taps, sine, None, f"{fs_in}->{fs_out} 1 kHz sine")
    # away from the ends the sine comes out as the sine (pass band flat within 0.15 dB, no delay)
    n = got.shape[1] - 5
    tt = np.arange(n) / fs_out
    mid = slice(n // 4, 3 * n // 4)
    assert np.abs(got[0, :n][mid] - 0.5 * np.sin(2 * np.pi * 1000.0 * tt)[mid]).max() < 0.5 * (10 ** (0.15 / 20) - 1)
    lengths = [1, 2, 37, 300, 4097, 10007, L, 0]
    batch = (rng.standard_normal((8, L)) * 0.3).astype(np.float32)
    check_rows(rs, taps, batch, lengths, f"{fs_in}->{fs_out} unequal lengths B=8")
    # rows that allow no 16-byte loads (odd offset and stride) give the same bits
    wide = cu(np.concatenate([np.zeros((8, 1), np.float32), batch, np.zeros((8, 2), np.float32)], 1))
    a = rs(wide[:, 1:1 + L], lengths=lengths, out=torch.full((8, RC.out_len(L, up, down)), SENTINEL, device="cuda"))
    b = rs(cu(batch), lengths=lengths, out=torch.full((8, RC.out_len(L, up, down)), SENTINEL, device="cuda"))
    assert torch.equal(a, b)


def test_sixteen_to_sixteen_copies(dev):
    from gtcrn_micro_amd._lib import Resampler
    x = torch.randn(3, 5000, device="cuda")
    assert torch.equal(Resampler(16000, 16000, 0)(x), x)


@pytest.mark.parametrize("fs", RC.OTHER_RATES)
def test_reference_clips_through_both_directions(dev, examples, fs):
    """Two seconds of two reference clips: brought to `fs` by the checker, then fs -> 16 kHz by the library against the
    checker on the same float32 samples; and 16 kHz -> fs by the library against the checker."""
    from gtcrn_micro_amd._lib import Resampler, resample_taps
    clip = examples["noisy"][:2, 40000:72000].astype(np.float32) / 32768.0
    upo, downo, _, ho = RC.design(16000, fs)
    at_fs = RC.resample64(clip, upo, downo, ho).astype(np.float32)
    check_rows(Resampler(fs, 16000, 0), resample_taps(fs, 16000), at_fs, None, f"clips {fs}->16000")
    check_rows(Resampler(16000, fs, 0), resample_taps(16000, fs), clip, None, f"clips 16000->{fs}")


@pytest.mark.parametrize("fs_in,fs_out", [(48000, 16000), (16000, 48000), (44100, 16000), (16000, 8000), (24000, 16000)])
def test_int16_forms_equal_the_float_form_between_the_pcm_conversions(dev, fs_in, fs_out):
    from gtcrn_micro_amd import pcm16_to_f32, f32_to_pcm16
    from gtcrn_micro_amd._lib import Resampler
    rs = Resampler(fs_in, fs_out, 0)
    gen = torch.Generator(device="cuda").manual_seed(fs_in)
    L = 8 * 1501
    lengths = [L, 3, 2000, 8191]
    x16 = torch.randint(-32768, 32768, (4, L), device="cuda", generator=gen, dtype=torch.int32).to(torch.int16)
    xf = pcm16_to_f32(x16)
    n = rs.out_len(L)
    ref = rs(xf, lengths=lengths, out=torch.zeros(4, n, device="cuda"))
    got = rs(x16, lengths=lengths, out=torch.zeros(4, n, device="cuda"))
    assert torch.equal(got, ref)                                                   # int16 in
    big = (torch.randn(4, L, device="cuda", generator=gen) * 0.7).contiguous()    # some samples clip
    yf = rs(big, out=torch.zeros(4, (n + 7) // 8 * 8, device="cuda"))
    y16 = rs(big, out=torch.zeros(4, (n + 7) // 8 * 8, device="cuda", dtype=torch.int16))
    assert torch.equal(y16, f32_to_pcm16(yf.contiguous()))                         # int16 out
    n1 = rs.out_len(L - 1)                                                          # rows off the 16-byte grid
    odd = rs(x16[:, 1:], lengths=[L - 1, 3, 2000, 8191], out=torch.zeros(4, n1, device="cuda"))
    assert torch.equal(odd, rs(xf[:, 1:].contiguous(), lengths=[L - 1, 3, 2000, 8191], out=torch.zeros(4, n1, device="cuda")))


def test_resampler_argument_errors(dev):
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import Resampler
    with pytest.raises(GtcrnError):
        Resampler(12345, 16000, 0)
    with pytest.raises(GtcrnError):
        Resampler(48000, 44100, 0)
    rs = Resampler(48000, 16000, 0)
    x = torch.zeros(2, 300, device="cuda")
    with pytest.raises(GtcrnError):
        rs(x.cpu())
    with pytest.raises(GtcrnError):
        rs(x.double())
    with pytest.raises(GtcrnError):
        rs(x, lengths=[1, 2, 3])
    with pytest.raises(GtcrnError):
        rs(x, lengths=[1, 301])
    with pytest.raises(GtcrnError):
        rs(x, out=torch.zeros(2, 99, device="cuda"))
    with pytest.raises(GtcrnError):
        rs(x.to(torch.int16), out=torch.zeros(2, 100, device="cuda", dtype=torch.int16))


# ---------------------------------------------------------------------------------- Engine.forward_wave_rate
@pytest.mark.parametrize("fs,out_fs", [(48000, None), (48000, 48000), (8000, 8000), (44100, 16000), (16000, 24000)])
def test_forward_wave_rate_is_the_three_public_calls_composed(eng, win, fs, out_fs):
    from gtcrn_micro_amd._lib import Resampler
    gen = torch.Generator(device="cuda").manual_seed(fs)
    x = torch.randn(3, fs // 2 + 13, device="cuda", generator=gen) * 0.1
    got = eng.forward_wave_rate(x, fs, win, out_fs=out_fs)
    mid = x if fs == 16000 else Resampler(fs, 16000, 0)(x)
    want = eng.forward_wave(mid, win)
    if out_fs not in (None, 16000):
        want = Resampler(16000, out_fs, 0)(want)
    assert torch.equal(got, want)
    assert torch.equal(eng.forward_wave_rate(x[0], fs, win, out_fs=out_fs), got[0])


@pytest.mark.parametrize("fs", [48000, 8000])
def test_end_to_end_against_the_float64_resampling_chain(eng, win, examples, fs):
    """The five reference clips (4 s each) at `fs` (made by the checker): forward_wave_rate(x, fs, out_fs=fs) against
    "checker resampler in float64 -> Engine.forward_wave -> checker resampler", rel_err <= TOL (1e-4).
    Measured on MI355X: 4.6e-07 at 48 kHz, 1.7e-06 at 8 kHz."""
    up, down, _, h = RC.design(fs, 16000)
    upo, downo, _, ho = RC.design(16000, fs)
    clip = examples["noisy"][:, 16000:80000].astype(np.float64) / 32768.0
    x = RC.resample64(clip, upo, downo, ho).astype(np.float32)
    mid = RC.resample64(x, up, down, h)
    ref16 = eng.forward_wave(cu(mid.astype(np.float32)), win).cpu().numpy()
    want = RC.resample64(ref16, upo, downo, ho)
    got = eng.forward_wave_rate(cu(x), fs, win, out_fs=fs).cpu().numpy()
    assert got.shape == want.shape
    e = rel_err(got, want)
    print(f"forward_wave_rate at {fs} Hz: rel_err {e:.3e} against the float64 resampling chain")
    assert e <= TOL
