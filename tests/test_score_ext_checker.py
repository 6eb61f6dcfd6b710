"""Pins tests/score_ext_checker.py, the float64 statement of ESTOI and segmental SNR that tests/test_gpu_score_ext.py
holds the kernels to: a second formulation of each metric, ESTOI's properties, and seeded wrong definitions that must
move the score far beyond anything the GPU test tolerates."""
import numpy as np
import pytest

import score_checker as SC
import score_ext_checker as SX

PARITY_CASES = ("L16000_B5", "L16000_B3", "var", "L64000_B1")      # the GPU test's parity inputs
GPU_CEILING = 5e-5                                                 # its ceiling, for ESTOI and for segmental SNR in dB


def parity_specs():
    return [sp for name in PARITY_CASES for sp in SC.GPU_CASES[name][1]]


def test_two_formulations_of_each_metric_agree():
    for sp in parity_specs():
        st = SC.case_reference(sp)["stages"]
        a, Sa = SX.estoi_from_envelopes(st["env_ref"], st["env_inf"])
        b, Sb = SX.estoi_from_envelopes_vectorised(st["env_ref"], st["env_inf"])
        assert Sa == Sb == SC.case_reference(sp)["segments"] and abs(a - b) <= 1e-12, sp
        ref, inf = SC.case_pair(sp)
        (v, F), (v2, F2) = SX.segsnr(ref, inf), SX.segsnr_vectorised(ref, inf)
        assert F == F2 == SX.segsnr_frames(len(ref))
        assert (F == 0 and v != v and v2 != v2) or abs(v - v2) <= 1e-12, sp
        got = SX.case_reference(sp)
        assert got["estoi"] == a and got["segsnr_frames"] == F and (got["segsnr"] == v or F == 0)
    assert any(SX.case_reference(sp)["segments"] == 0 for sp in parity_specs())        # the constant path is among them


def test_estoi_ignores_positive_scaling_of_either_signal():
    ref, inf = SC.case_pair(SC.GPU_CASES["L16000_B3"][1][0])
    want = SX.estoi(ref, inf)
    assert 0.0 < want < 1.0
    for a, b in ((0.25, 1.0), (1.0, 3.0), (0.5, 0.125)):                # (powers of two and 3: exact in float32 or not)
        got = SX.estoi(np.float32(a) * ref, np.float32(b) * inf)
        assert abs(got - want) <= 1e-6, (a, b, got, want)


def test_estoi_is_one_for_identical_signals_and_zero_for_silence():
    x = SC.excerpt_pair(SC.examples(), 1, 8, 16000)[0]
    z = np.zeros_like(x)
    assert abs(SX.estoi(x, x) - 1.0) <= 1e-9
    assert SX.estoi(z, x) == 0.0 and SX.estoi(x, z) == 0.0 and SX.estoi(z, z) == 0.0


def test_estoi_is_monotone_on_the_snr_ladder():
    got = [SX.estoi(*SC.ladder_pair(SC.examples(), snr)) for snr in SC.SNR_LADDER]
    print(got)
    assert all(b > a for a, b in zip(got, got[1:])) and 0.0 < got[0] and got[-1] < 1.0


def test_segsnr_of_silence_and_identity():
    x = SC.excerpt_pair(SC.examples(), 1, 8, 16000)[0]
    z = np.zeros_like(x)
    assert SX.segsnr(z, x)[0] == -10.0 and SX.segsnr(z, z)[0] == -10.0 and SX.segsnr(x, x)[0] == 35.0
    assert abs(SX.segsnr(x, z)[0]) <= 1e-6


@pytest.mark.parametrize("bug", ["no_columns", "clipped"])
def test_a_wrong_estoi_definition_moves_the_score(bug):
    moved = []
    for sp in parity_specs():
        want = SX.case_reference(sp)
        if want["segments"] == 0:
            continue
        st = want["stages"]
        moved.append(abs(SX.estoi_wrong(st["env_ref"], st["env_inf"], bug) - want["estoi"]))
    print(bug, moved)
    # One clip beyond the bound fails the GPU parity test, which runs them all.  (ESTOI ignores alpha, and the clipping
    # acts only where inf exceeds ref by 15 dB in a band: on the gated clips, not on every one.)
    assert len(moved) >= 10 and max(moved) > 100 * GPU_CEILING


@pytest.mark.parametrize("bug", ["hop128", "drop_last"])
def test_a_wrong_segsnr_definition_moves_the_score(bug):
    moved = []
    for sp in parity_specs():
        want = SX.case_reference(sp)
        if want["segsnr_frames"] < 2:
            continue
        moved.append(abs(SX.segsnr_wrong(*SC.case_pair(sp), bug) - want["segsnr"]))
    print(bug, moved)
    # one clip beyond the bound fails the GPU parity test, which runs them all
    assert len(moved) >= 10 and max(moved) > 100 * GPU_CEILING


def test_segsnr_frame_counts_at_the_edges():
    rng = np.random.default_rng(5)
    for n, F in ((0, 0), (1, 0), (479, 0), (480, 1), (599, 1), (600, 2), (720, 3), (64000, 530)):
        assert SX.segsnr_frames(n) == F, n
        x = rng.standard_normal(n).astype(np.float32)
        y = (x + 0.1 * rng.standard_normal(n)).astype(np.float32)
        v, got = SX.segsnr(x, y)
        assert got == F and (np.isfinite(v) if F else v != v)
    w = SX.segsnr_window()
    assert w.size == 480 and np.allclose(w, w[::-1], atol=1e-15) and w.min() > 0.0 and abs(w.max() - 1.0) < 2e-5
