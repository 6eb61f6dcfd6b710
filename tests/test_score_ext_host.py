"""CPU-side checks of the "scores, extended" section of include/gtcrn_micro_hip.h: the exported symbols, the 64-byte
record, the host-only segmental-SNR functions against the float64 checker, and the ext workspace size."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import score_ext_checker as SX

EXT_SYMBOLS = ["gtcrn_score_ext_workspace_bytes", "gtcrn_score_ext", "gtcrn_score_segsnr_frames",
               "gtcrn_score_segsnr_window", "gtcrn_score_ext_stages", "gtcrn_score_ext_timing_read"]
ERR_ARG = -1


class Record(ctypes.Structure):
    _fields_ = [("sdr", ctypes.c_double), ("sisnr", ctypes.c_double), ("stoi", ctypes.c_double),
                ("kept_frames", ctypes.c_int), ("segments", ctypes.c_int)]


class ExtRecord(ctypes.Structure):
    _fields_ = [("base", Record), ("estoi", ctypes.c_double), ("segsnr", ctypes.c_double),
                ("segsnr_frames", ctypes.c_int), ("zero", ctypes.c_int * 3)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def test_ext_symbols_exported_declared_and_abi_version_unchanged():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    header = open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")).read()
    from gtcrn_micro_amd import _lib
    for n in EXT_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\b%s\(" % n, header), f"{n} is not declared in the header"
        assert getattr(_lib.lib(), n).argtypes is not None, f"{n} has no ctypes declaration"
    assert "gtcrn_score_ext_record" in header
    assert L.gtcrn_abi_version() == 1
    assert "#define GTCRN_ABI_VERSION 1" in header
    assert _lib.lib().gtcrn_score_ext_stages() == 9


def test_the_ext_record_is_64_bytes_with_the_old_record_in_front():
    assert ctypes.sizeof(Record) == 32 and ctypes.sizeof(ExtRecord) == 64
    assert (ExtRecord.base.offset, ExtRecord.estoi.offset, ExtRecord.segsnr.offset, ExtRecord.segsnr_frames.offset,
            ExtRecord.zero.offset) == (0, 32, 40, 48, 52)


def test_segsnr_frames_and_window_are_the_checkers():
    from gtcrn_micro_amd._lib import lib
    for n in (0, 1, 479, 480, 599, 600, 601, 719, 720, 5399, 16000, 40001, 64000, 1 << 28):
        assert lib().gtcrn_score_segsnr_frames(n) == SX.segsnr_frames(n), n
    assert lib().gtcrn_score_segsnr_frames(-1) == ERR_ARG and lib().gtcrn_score_segsnr_frames((1 << 28) + 1) == ERR_ARG
    w = (ctypes.c_double * 480)()
    assert lib().gtcrn_score_segsnr_window(w) == 0
    # cos of the C library and of numpy may differ in the last place
    assert np.abs(np.array(w) - SX.segsnr_window()).max() <= 2.0 ** -52
    assert lib().gtcrn_score_segsnr_window(None) == ERR_ARG


def test_ext_workspace_bytes_hold_the_old_workspace_and_are_linear_in_b():
    from gtcrn_micro_amd._lib import lib
    f, old = lib().gtcrn_score_ext_workspace_bytes, lib().gtcrn_score_workspace_bytes
    Ls = (1, 257, 480, 6000, 16000, 40001, 64000, 496000)
    one = [f(1, L) for L in Ls]
    assert all(v > 0 and v % 16 == 0 for v in one)
    assert all(b >= a for a, b in zip(one, one[1:]))
    for L, v in zip(Ls, one):
        # the old slice, a 32-byte record, a double per segment and a double per segmental-SNR frame
        segs = max(lib().gtcrn_score_frames(L) - 1 - 29, 0)
        assert v >= old(1, L) + 32 + 8 * segs + 8 * SX.segsnr_frames(L), L
    for B in (2, 5, 256):
        assert [f(B, L) for L in Ls] == [B * v for v in one]          # a clip's share is a function of L alone
    for B, L in ((0, 16000), (65536, 16000), (1, 0), (1, (1 << 28) + 1)):
        assert f(B, L) == 0, (B, L)
        assert b"gtcrn_score_ext_workspace_bytes" in lib().gtcrn_last_error()


def test_score_ext_refuses_a_null_scorer_before_touching_a_device():
    from gtcrn_micro_amd._lib import lib
    assert lib().gtcrn_score_ext(None, None, 0, None, 0, None, 16000, 1, 31, None, None, None) == ERR_ARG
    t = ctypes.c_float()
    assert lib().gtcrn_score_ext_timing_read(None, 0, None, 0, ctypes.byref(t)) == ERR_ARG
