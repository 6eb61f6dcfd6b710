"""Pins tests/score_checker.py, the float64 statement of the "scores" contract the GPU tests hold the kernels to:
against the reference's own SDR / SI-SNR numbers (tests/golden/score_ref.npz), against what STOI promises, and the
condition its inputs must meet before a keep mask can be compared exactly."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import score_checker as SC


@pytest.fixture(scope="module")
def ex():
    return SC.examples()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "score_ref.npz"))


def golden_pairs(ex, gold):
    assert [tuple(e) for e in gold["excerpts"]] == list(SC.EXCERPTS) and tuple(gold["snr_ladder"]) == SC.SNR_LADDER
    return [SC.excerpt_pair(ex, c, o) for c, o in SC.EXCERPTS] + [SC.ladder_pair(ex, s) for s in SC.SNR_LADDER]


def test_checker_reproduces_the_references_numbers_to_the_recorded_floor(ex, gold):
    """sdr_metric / sisnr_metric of the reference ran in float32 on these pairs; the float64 checker differs from them by
    the reference's own rounding, recorded in MANIFEST_score.json when the numbers were taken."""
    man = json.load(open(os.path.join(GOLDEN, "MANIFEST_score.json")))
    pairs = golden_pairs(ex, gold)
    d_sdr = max(abs(SC.sdr(r, y) - g) for (r, y), g in zip(pairs, gold["sdr"]))
    d_sisnr = max(abs(SC.sisnr(r, y) - g) for (r, y), g in zip(pairs, gold["sisnr"]))
    print(f"max |reference float32 - checker float64|: SDR {d_sdr:.3e} dB, SI-SNR {d_sisnr:.3e} dB")
    # the recorded floor, and a float32 sum of 64000 terms is good to a few 1e-6 relative: far below 1e-4 dB
    assert d_sdr <= man["sdr_reference_float32_vs_checker_float64_max_db"] * 1.001 + 1e-9
    assert d_sisnr <= man["sisnr_reference_float32_vs_checker_float64_max_db"] * 1.001 + 1e-9
    assert max(man["sdr_reference_float32_vs_checker_float64_max_db"],
               man["sisnr_reference_float32_vs_checker_float64_max_db"]) < 1e-4


def test_band_table_and_resampler_follow_the_definition():
    lo, hi = SC.bands()
    assert tuple(lo) == SC.BAND_LO == (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174)
    assert tuple(hi) == SC.BAND_HI == (9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)
    h = SC.design_taps()
    assert h.size == 513 and abs(h.sum() - 5.0) < 1e-12 and np.array_equal(h, h[::-1])
    x = np.random.default_rng(3).standard_normal(333)
    y = SC.resample10(x)
    assert y.size == -(-333 * 5 // 8)
    assert np.abs(y - SC.resample10_direct(x)).max() < 1e-13     # resample_poly == the header's sum, term by term
    assert [SC.frames(L) for L in (257, 409, 410, 411, 6000, 16000, 64000)] == [0, 0, 1, 1, 28, 77, 311]   # 410 samples -> 257 at 10 kHz -> one frame


def test_stoi_of_a_signal_with_itself_is_one(ex):
    r, _ = SC.excerpt_pair(ex, 0, 8)
    assert abs(SC.stoi(r, r) - 1.0) < 1e-12


def test_stoi_rises_strictly_with_snr(ex):
    vals = [SC.stoi(*SC.ladder_pair(ex, s)) for s in SC.SNR_LADDER]
    print("STOI over", SC.SNR_LADDER, "dB:", np.round(vals, 4))
    assert all(b > a for a, b in zip(vals, vals[1:])), vals
    assert 0.0 < vals[0] and vals[-1] < 1.0


def test_common_scale_acts_as_the_formulas_imply(ex):
    """STOI normalises every segment, so a common gain g leaves it alone (up to EPS).  SDR and SI-SNR are ratios of sums
    that both scale by g^2, so they move through their 1e-8 terms alone, and by exactly what the formulas say."""
    r, y = SC.excerpt_pair(ex, 2, 8)
    r64, y64 = r.astype(np.float64), y.astype(np.float64)
    rc, yc = r64 - r64.mean(), y64 - y64.mean()
    rr, dd, dot, n = np.sum(rc ** 2), np.sum((yc - rc) ** 2), np.sum(yc * rc), r64.size
    for g in (0.25, 4.0, 2.0 ** -20):          # powers of two: the scaled float64 signals are exact
        g2 = g * g
        if g2 * rr > 1e-3:
            assert abs(SC.stoi(g * r64, g * y64) - SC.stoi(r64, y64)) < 1e-10
        want_sdr = 10 * np.log10((g2 * rr + 1e-8) / (g2 * dd + 1e-8))
        a = g2 * dot / (g2 * rr + n * 1e-8)
        want_sisnr = 10 * np.log10((a * a * rr * g2 + 1e-8) / (g2 * np.sum((yc - a * rc) ** 2) + 1e-8))
        assert abs(SC.sdr(g * r64, g * y64) - want_sdr) < 1e-9
        assert abs(SC.sisnr(g * r64, g * y64) - want_sisnr) < 1e-9
    assert abs(SC.sdr(2.0 ** -20 * r64, 2.0 ** -20 * y64) - SC.sdr(r64, y64)) > 1.0    # ... and at 2^-20 they are not


def test_short_clips_give_pystois_constant(ex):
    r, y = SC.excerpt_pair(ex, 0, 0, 6000)              # 28 frames: fewer than 31 kept
    s = SC.score(r, y)
    assert s["stoi"] == 1e-5 and s["segments"] == 0 and s["kept_frames"] == 28
    r, y = SC.excerpt_pair(ex, 0, 0, 257)               # no analysis frame at all
    s = SC.score(r, y)
    assert s["stoi"] == 1e-5 and s["segments"] == 0 and s["kept_frames"] == 0
    n31 = next(L for L in range(6000, 8000) if SC.frames(L) == 31)
    r, y = SC.excerpt_pair(ex, 3, 8, n31)               # 31 kept frames -> M = 30 -> one segment
    s = SC.score(r, y)
    assert s["kept_frames"] == 31 and s["segments"] == 1 and s["stoi"] != 1e-5


def test_silence_keeps_every_score_defined():
    z = np.zeros(16000, np.float32)
    x = (np.random.default_rng(5).standard_normal(16000) * 0.1).astype(np.float32)
    for r, y in ((z, x), (x, z), (z, z)):
        s = SC.score(r, y)
        assert np.isfinite([s["sdr"], s["sisnr"], s["stoi"]]).all(), s
        assert s["kept_frames"] == SC.frames(16000)
    assert SC.score(z, z)["sdr"] == 0.0 and SC.score(z, x)["stoi"] == 0.0


def test_gpu_mask_inputs_stay_clear_of_the_threshold():
    """The GPU test compares keep masks exactly.  That is fair only where no frame energy lies near max - 40 dB: the
    kernels resample and frame in fp32-rounded samples, which moves an energy 40 dB below the maximum by about 1e-4 dB;
    0.01 dB leaves about 100 x."""
    specs = [sp for _, clips in SC.GPU_CASES.values() for sp in clips]
    assert len(set(specs)) >= 8
    dropped = 0
    for sp in specs:
        st = SC.case_reference(sp)["stages"]
        print(sp, f"frames {st['n']} kept {st['kept_frames']} nearest energy to the threshold {st['margin_db']:.4f} dB")
        assert st["margin_db"] > SC.MASK_MARGIN_DB, sp
        dropped += st["n"] - st["kept_frames"]
    assert dropped > 100        # the masks are not all trivial: the gated references lose whole runs of frames
