"""CPU-side checks of the "scores" section of include/gtcrn_micro_hip.h: the exported symbols, the host-only design
functions against the float64 checker, the workspace size, and that the 16 kHz -> 10 kHz stage did not become a rate of
the public resampler."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import score_checker as SC

SCORE_SYMBOLS = ["gtcrn_scorer_create", "gtcrn_scorer_destroy", "gtcrn_score_workspace_bytes", "gtcrn_score",
                 "gtcrn_score_taps", "gtcrn_score_bands", "gtcrn_score_frames", "gtcrn_score_debug",
                 "gtcrn_score_timing", "gtcrn_score_timing_read"]
ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def test_score_symbols_exported_declared_and_abi_version_unchanged():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    header = open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")).read()
    from gtcrn_micro_amd import _lib
    for n in SCORE_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\b%s\(" % n, header), f"{n} is not declared in the header"
        assert getattr(_lib.lib(), n).argtypes is not None, f"{n} has no ctypes declaration"
    assert L.gtcrn_abi_version() == 1
    assert "#define GTCRN_ABI_VERSION 1" in header
    assert ctypes.sizeof(ctypes.c_double) * 3 + ctypes.sizeof(ctypes.c_int) * 2 == 32      # the record


def test_band_tables_are_the_checkers():
    from gtcrn_micro_amd import score_bands
    lo, hi = score_bands()
    assert tuple(lo) == SC.BAND_LO and tuple(hi) == SC.BAND_HI
    assert (lo, hi) == SC.bands()


def test_taps_are_the_checkers_design_after_one_float_rounding():
    from gtcrn_micro_amd import score_taps
    up, down, h = score_taps()
    assert (up, down) == (5, 8) and h.dtype == np.float32 and h.size == 513
    assert np.array_equal(h, SC.design_taps().astype(np.float32))
    assert abs(float(h.astype(np.float64).sum()) - 5.0) <= 5e-6
    assert np.array_equal(h, h[::-1]) and not np.any(h == 0.0)


def test_taps_refuse_a_short_buffer():
    from gtcrn_micro_amd._lib import lib
    buf = (ctypes.c_float * 16)()
    assert lib().gtcrn_score_taps(None, None, buf, 16) == ERR_ARG
    assert lib().gtcrn_score_taps(None, None, None, 0) == 513


def test_frames_match_the_checker():
    from gtcrn_micro_amd import score_frames
    for L in (0, 1, 256, 257, 409, 410, 411, 6000, 16000, 40001, 64000, 496000, 1 << 28):
        assert score_frames(L) == SC.frames(L), L
    from gtcrn_micro_amd._lib import lib
    assert lib().gtcrn_score_frames(-1) == ERR_ARG


def test_the_public_resampler_still_refuses_10_khz():
    from gtcrn_micro_amd._lib import lib
    up, down = ctypes.c_int(), ctypes.c_int()
    assert lib().gtcrn_resample_taps(16000, 10000, ctypes.byref(up), ctypes.byref(down), None, 0) == ERR_ARG
    assert lib().gtcrn_resample_out_len(16000, 10000, 1000) == ERR_ARG
    h = ctypes.c_void_p()
    assert lib().gtcrn_resampler_create(ctypes.byref(h), 16000, 10000, 0) == ERR_ARG and not h.value


def test_workspace_bytes_are_monotone_and_linear_in_b():
    from gtcrn_micro_amd._lib import lib
    f = lib().gtcrn_score_workspace_bytes
    Ls = (1, 257, 411, 6000, 16000, 40001, 64000, 496000)
    one = [f(1, L) for L in Ls]
    assert all(v > 0 and v % 16 == 0 for v in one)
    assert all(b >= a for a, b in zip(one, one[1:]))
    for B in (2, 5, 256):
        assert [f(B, L) for L in Ls] == [B * v for v in one]          # a clip's slice is a function of L alone
    # room for both 10 kHz signals and both envelope sets at least
    assert f(1, 64000) >= 4 * (2 * 40000 + 2 * 15 * 310)
    assert f(0, 16000) == 0 and f(1, 0) == 0 and f(1, (1 << 28) + 1) == 0


def test_score_refuses_bad_arguments_before_touching_a_device():
    """A null scorer is refused first, so this needs no GPU."""
    from gtcrn_micro_amd._lib import lib
    assert lib().gtcrn_score(None, None, 0, None, 0, None, 16000, 1, 7, None, None, None) == ERR_ARG
    assert lib().gtcrn_score_debug(None, 0, 0, None, 0, None) == ERR_ARG
    assert lib().gtcrn_score_bands(None, None) == ERR_ARG


def test_rank_score_files_merge_like_the_scp_lists(tmp_path):
    """write_scores per rank, merge_scores on rank 0: the merged files are what one rank would have written for all."""
    from gtcrn_micro_amd.infer import merge_scores, write_scores
    rows = [(f"clip{k}", {"SDR": 10.0 + k / 3.0, "SISNR": 9.5 - k / 7.0, "STOI": 0.5 + k / 100.0}) for k in range(5)]
    rows[3][1]["STOI"] = float("nan")
    skipped = [("clip9", "clip at 8000 Hz")]
    one, many = tmp_path / "one", tmp_path / "many"
    one.mkdir()
    many.mkdir()
    write_scores(str(one), rows, skipped)
    write_scores(str(many), rows[:2], [], ".rank0")
    write_scores(str(many), rows[2:], skipped, ".rank1")
    merge_scores(str(many), 2)
    for name in ("SDR.scp", "SISNR.scp", "STOI.scp", "RESULTS.txt"):
        assert open(one / name).read() == open(many / name).read(), name
    lines = open(one / "RESULTS.txt").read().splitlines()
    assert lines[0] == "SDR: %.4f" % np.mean([r[1]["SDR"] for r in rows])
    assert lines[2] == "STOI: %.4f" % np.nanmean([r[1]["STOI"] for r in rows]) and lines[3].startswith("SKIPPED: clip9 (clip at 8000 Hz")
    assert open(one / "SDR.scp").read().splitlines()[1] == f"clip1 {rows[1][1]['SDR']!r}"
