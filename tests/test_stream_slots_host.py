"""CPU-side checks of the stream-slot entry points (gtcrn_*_slots): the six symbols exist and are declared, the ABI version
and both state sizes are what they were, and a call without a model is an argument error before the device is touched."""
import ctypes
import os

import pytest

from conftest import ROOT

import __graft_entry__ as graft

torch = pytest.importorskip("torch")

SLOT_SYMBOLS = ["gtcrn_stream_step_slots", "gtcrn_stream_reset_slots", "gtcrn_wave_stream_step_slots",
                "gtcrn_wave_stream_step_slots_pcm16", "gtcrn_wave_stream_flush_slots", "gtcrn_wave_stream_flush_slots_pcm16"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def test_slot_symbols_exported_and_declared():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    with open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")) as f:
        header = f.read()
    for n in SLOT_SYMBOLS:
        assert hasattr(L, n), n
        assert f"int {n}(gtcrn_model *m" in header, n


def test_abi_version_and_state_sizes_unchanged():
    from gtcrn_micro_amd import Engine
    from gtcrn_micro_amd._lib import lib
    assert lib().gtcrn_abi_version() == 1
    assert Engine.state_bytes() == 4 * 38116 == 152464
    assert Engine.wave_state_bytes() == 4 * (512 + 256 + 4) == 3088


def test_null_model_is_an_argument_error():
    from gtcrn_micro_amd._lib import lib
    L = lib()
    p = ctypes.c_void_p(16)           # never dereferenced: every call below is rejected before the device is touched
    ERR_ARG = -1
    calls = [
        lambda: L.gtcrn_stream_step_slots(None, p, p, p, 4, p, 514, 2, 2, p, 514, 2, 2, None),
        lambda: L.gtcrn_stream_reset_slots(None, p, p, p, p, 4, None),
        lambda: L.gtcrn_wave_stream_step_slots(None, p, p, p, p, 4, p, 256, p, 256, None, p, None),
        lambda: L.gtcrn_wave_stream_step_slots_pcm16(None, p, p, p, p, 4, p, 256, p, 256, None, p, None),
        lambda: L.gtcrn_wave_stream_flush_slots(None, p, p, p, p, 4, p, 256, 10, p, 256, None, p, None),
        lambda: L.gtcrn_wave_stream_flush_slots_pcm16(None, p, p, p, p, 4, p, 256, 10, p, 256, None, p, None),
    ]
    for i, c in enumerate(calls):
        assert c() == ERR_ARG, i
        assert b"null model" in L.gtcrn_last_error(), i
